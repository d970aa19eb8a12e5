"""Minimizer seeding without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, struct BaSeedingParams is
12 bytes, every argument rejection is reported before the device is touched, and the kernels compile for gfx950 without scratch. One
rejection is not here: ba_chaining_create_seeded on a seeder that has not run needs a seeder, which cannot be created without a device; it
is checked in tests/test_gpu_seeding.py::test_reload_with_a_smaller_set_and_back (a null seeder is refused here)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chaining_ref, seeding_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_seeding_create", "ba_seeding_reload", "ba_seeding_run", "ba_seeding_counts", "ba_seeding_results", "ba_seeding_sketch",
         "ba_seeding_times", "ba_seeding_destroy", "ba_chaining_create_seeded")
CALLER = r"""
#include "block_aligner_hip.h"
typedef char params_are_12_bytes[sizeof(struct BaSeedingParams) == 12 ? 1 : -1];
int use(const uint8_t* pool, const uint64_t* off, const uint32_t* len, const uint8_t* strand) {
    struct BaSeedingParams p = {15, 10, 64};
    struct BaChainingParams cp = {4, 1, 0, 64, 500, 100, 3, 20, 1};
    BaSeeding* b = ba_seeding_create(&p, pool, off, len, off, len, strand, 1);
    float ms = 0.0f, a, s, m;
    uint64_t nh, nq, nr, first[2], qf[2], rf[2]; uint32_t per[1], q[8], r[8], l[8], qp[8], qc[8], rp[8], rc[8];
    BaChaining* c;
    int rc_ = ba_seeding_reload(b, pool, off, len, off, len, NULL, 1);
    rc_ |= ba_seeding_run(b, &ms);
    rc_ |= ba_seeding_counts(b, &nh, &nq, &nr, per);
    rc_ |= ba_seeding_results(b, first, q, r, l);
    rc_ |= ba_seeding_sketch(b, qf, qp, qc, rf, rp, rc);
    rc_ |= ba_seeding_times(b, &a, &s, &m);
    rc_ |= ba_seeding_times(b, NULL, NULL, NULL);
    c = ba_chaining_create_seeded(&cp, b);
    rc_ |= ba_chaining_run(c, &ms);
    ba_chaining_destroy(c);
    ba_seeding_destroy(b);
    return rc_;
}
"""
GOOD = S.Params(5, 4, 2)


def test_seeding_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_seeding_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)   # (holds the size of the struct as a compile-time check)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_params_are_three_4_byte_fields(hip):
    assert ctypes.sizeof(hip.SeedingParamsC) == 12
    assert [f[0] for f in hip.SeedingParamsC._fields_] == list(S.Params._fields)
    assert all(ctypes.sizeof(f[1]) == 4 for f in hip.SeedingParamsC._fields_)


def _set():
    """Two problems: the first known answer, and the second one on the minus strand."""
    return S.ProblemSet([(S.KNOWN_Q, S.KNOWN_R, 0), (S.KNOWN_Q_MINUS, S.KNOWN_R, 1)])


def _make(hip, P=GOOD, **over):
    ps = _set()
    a = dict(pool=ps.pool, q_off=ps.q_off, q_len=ps.q_len, r_off=ps.r_off, r_len=ps.r_len, strand=ps.strand)
    a.update(over)
    return hip.Seeder(*P, a["pool"], a["q_off"], a["q_len"], a["r_off"], a["r_len"], a["strand"])


def _no_device(hip):
    try:
        return hip.device_count() < 1
    except Exception:
        return True


def _accepted(hip, *args, **kw):
    """The set passes every check: without a device it gets as far as the device."""
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            _make(hip, *args, **kw)
    else:
        _make(hip, *args, **kw).close()


def test_a_valid_set_passes_every_check(hip):
    _accepted(hip)
    _accepted(hip, strand=None)


def test_accepts_the_limits_of_the_parameters(hip):
    for P in (S.Params(4, 1, 1), S.Params(16, 64, S.NO_CAP)):
        _accepted(hip, P)


@pytest.mark.parametrize("change, message", [
    (dict(k=3), r"k must be between 4 and 16 \(it is 3\)"),
    (dict(k=17), r"k must be between 4 and 16 \(it is 17\)"),
    (dict(w=0), r"w must be between 1 and 64 \(it is 0\)"),
    (dict(w=65), r"w must be between 1 and 64 \(it is 65\)"),
    (dict(max_occ=0), "max_occ must be at least 1"),
])
def test_rejects_parameters_out_of_range(hip, change, message):
    with pytest.raises(RuntimeError, match=message):
        _make(hip, GOOD._replace(**change))


def test_rejects_a_sequence_of_2_31_minus_16_bytes(hip):
    """(Only the length is read before the rejection: no such pool exists here.)"""
    ps = _set()
    for side in ("q_len", "r_len"):
        L = getattr(ps, side).copy()
        L[1] = (1 << 31) - 16
        with pytest.raises(RuntimeError, match=r"problem 1: the sequences .* must be shorter than 2\^31 - 16 bytes"):
            _make(hip, **{side: L})
        L[1] = 0xffffffff
        with pytest.raises(RuntimeError, match=r"problem 1: the sequences"):
            _make(hip, **{side: L})


def test_rejects_a_bad_strand(hip):
    with pytest.raises(RuntimeError, match="problem 1: strand must be 0 or 1"):
        _make(hip, strand=np.array([0, 2], np.uint8))


def test_rejects_mismatched_arrays(hip):
    ps = _set()
    with pytest.raises(ValueError, match="one entry per problem"):
        _make(hip, q_len=ps.q_len[:1])
    with pytest.raises(ValueError, match="one entry per problem"):
        _make(hip, r_off=np.zeros(3, np.uint64))
    with pytest.raises(ValueError, match="one entry per problem"):
        _make(hip, strand=np.zeros(1, np.uint8))


def test_rejects_an_empty_set(hip):
    z = np.zeros(0, np.uint32)
    with pytest.raises(RuntimeError, match="between 1 and 2\\^28 problems"):
        hip.Seeder(*GOOD, np.zeros(4, np.uint8), z, z, z, z)


def test_null_batches_and_null_arguments_are_refused(hip):
    L = hip.lib()
    ms = ctypes.c_float()
    assert L.ba_seeding_run(None, ctypes.byref(ms)) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_counts(None, None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_results(None, *([None] * 4)) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_sketch(None, *([None] * 6)) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_times(None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_reload(None, *([None] * 6), 0) != 0 and "null batch" in hip.last_error()
    L.ba_seeding_destroy(None)
    CP = hip.ChainingParamsC(*chaining_ref.E2E_PARAMS)
    assert not L.ba_chaining_create_seeded(ctypes.byref(CP), None) and "null batch" in hip.last_error()
    one = np.zeros(2, np.uint64)
    assert not L.ba_chaining_create_seeded(None, one.ctypes.data) and "null argument" in hip.last_error()
    P = hip.SeedingParamsC(*GOOD)
    assert not L.ba_seeding_create(None, *([one.ctypes.data] * 5), None, 1) and "null argument" in hip.last_error()
    for k in range(5):
        args = [one.ctypes.data] * 5
        args[k] = None
        assert not L.ba_seeding_create(ctypes.byref(P), *args, None, 1) and "null argument" in hip.last_error(), k


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_seeding_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_seeding.hip"), "-o", str(tmp_path / "ba_seeding.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scratch = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 5 and set(scratch.values()) == {0}, scratch   # every kernel of the unit: two passes of the sketch and the match, the sort
    for k, passes in (("k_seeding_sketch", 2), ("k_seeding_sort", 1), ("k_seeding_match", 2)):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0] * passes, (k, scratch)


def test_kernel_hash_and_makefile_list_the_seeding_sources():
    from tools import kernel_hash
    assert "ba_seeding.hip" in kernel_hash.FILES and "ba_seeding.h" in kernel_hash.FILES
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    assert re.search(r"^XOBJS := .*\$\(OBJ\)/ba_seeding\.o", mk, flags=re.M) and re.search(r"^HDRS := .*\bba_seeding\.h\b", mk, flags=re.M)
    launch = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_launch.h")).read()
    for f in ("ba_launch_seeding_sketch", "ba_launch_seeding_sort", "ba_launch_seeding_match"):
        assert f in launch
