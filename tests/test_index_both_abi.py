"""Both strands at once without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, every rejection
arrives with its message before a device is needed, and the new kernels are a unit of their own that builds for gfx950 without scratch.
ba_seeding_create_indexed_both looks at its index last, so its other arguments are judged here with a null index; the refusals of mixed
use need an index or a seeder and are in tests/test_gpu_index_both.py::test_mixed_use_is_refused."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import index_both_ref as B, seeding_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_ref_index_create_canonical", "ba_ref_index_is_canonical", "ba_seeding_create_indexed_both", "ba_seeding_reload_indexed_both",
         "ba_seeding_problems")
CALLER = r"""
#include "block_aligner_hip.h"
int use(const uint8_t* pool, const uint64_t* off, const uint32_t* len, const struct BaChainingParams* P) {
    BaRefIndex* x = ba_ref_index_create_canonical(15, 10, pool, off, len, 3);
    uint64_t n_problems, n_reads, first[5], q_first[3]; uint32_t code[8], pos[8], q[8], r[8], l[8], per[4]; int flag;
    BaSeeding* s = ba_seeding_create_indexed_both(x, 64, 0xffffffffu, pool, off, len, 2);
    BaChaining* c;
    int rc = ba_ref_index_is_canonical(x, &flag);
    rc |= ba_ref_index_is_canonical(x, NULL);
    rc |= ba_ref_index_entries(x, code, pos);
    ba_ref_index_destroy(x);
    rc |= ba_seeding_reload_indexed_both(s, pool, off, len, 1);
    rc |= ba_seeding_problems(s, &n_problems, &n_reads);
    rc |= ba_seeding_problems(s, NULL, NULL);
    rc |= ba_seeding_run(s, NULL);
    rc |= ba_seeding_counts(s, NULL, NULL, NULL, per);
    rc |= ba_seeding_results(s, first, q, r, l);
    rc |= ba_seeding_sketch(s, q_first, pos, code, NULL, NULL, NULL);
    c = ba_chaining_create_seeded(P, s);
    ba_chaining_destroy(c); ba_seeding_destroy(s);
    return rc + (pos[0] >> 31);
}
"""
LIMIT = 0x7fffffff - 16


def test_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    header = open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read()
    assert "strand in bit 31" in header   # what ba_ref_index_entries returns for such an index


def _no_device(hip):
    try:
        return hip.device_count() < 1
    except Exception:
        return True


def _accepted(hip, make):
    """The arguments pass every check: without a device they get as far as the device."""
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            make()
    else:
        make().close()


# ------------------------------------------------------------------ ba_ref_index_create_canonical: create_multi's checks and messages
def test_valid_sequences_pass_every_check(hip):
    _accepted(hip, lambda: hip.RefIndex.from_sequences(5, 4, [S.KNOWN_R, b"", S.KNOWN_R[:3]], canonical=True))
    _accepted(hip, lambda: hip.RefIndex.from_sequences(16, 64, [b""], canonical=True))
    _accepted(hip, lambda: hip.RefIndex(4, 1, S.KNOWN_R, canonical=True))
    _accepted(hip, lambda: hip.RefIndex(15, 10, b"", canonical=True))
    pool = np.frombuffer(b"##" + S.KNOWN_R + b"#" + S.KNOWN_Q, np.uint8)   # apart, and not in order
    _accepted(hip, lambda: hip.RefIndex.from_sequences(5, 4, pool, [3 + len(S.KNOWN_R), 2, 0], [len(S.KNOWN_Q), len(S.KNOWN_R), 0], canonical=True))


def test_create_canonical_refusals(hip):
    L = hip.lib()
    one = np.zeros(8, np.uint64)
    for k in range(3):
        args = [one.ctypes.data] * 3
        args[k] = None
        assert not L.ba_ref_index_create_canonical(5, 4, *args, 1) and "null argument" in hip.last_error(), k
    for k, w, message in ((3, 4, r"k must be between 4 and 16 \(it is 3\)"), (17, 4, r"k must be between 4 and 16 \(it is 17\)"),
                          (5, 0, r"w must be between 1 and 64 \(it is 0\)"), (5, 65, r"w must be between 1 and 64 \(it is 65\)")):
        with pytest.raises(RuntimeError, match=message):
            hip.RefIndex.from_sequences(k, w, [S.KNOWN_R], canonical=True)
        with pytest.raises(RuntimeError, match=message):
            hip.RefIndex(k, w, S.KNOWN_R, canonical=True)
    with pytest.raises(RuntimeError, match=r"between 1 and 2\^20 sequences \(it has 0\)"):
        hip.RefIndex.from_sequences(5, 4, [], canonical=True)
    n = (1 << 20) + 1
    with pytest.raises(RuntimeError, match=rf"between 1 and 2\^20 sequences \(it has {n}\)"):
        hip.RefIndex.from_sequences(5, 4, np.zeros(8, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32), canonical=True)
    lens = np.array([1 << 30, (1 << 30) - 17, 0], np.uint32)   # (only the lengths are read before the refusal: no such sequences exist here)
    assert not L.ba_ref_index_create_canonical(5, 4, one.ctypes.data, one.ctypes.data, lens.ctypes.data, 3)
    assert re.search(rf"the sequences \({LIMIT} bytes in all\) must be shorter than 2\^31 - 16 bytes", hip.last_error())
    assert L.ba_ref_index_is_canonical(None, None) != 0 and "null index" in hip.last_error()


# ------------------------------------------------------------------ ba_seeding_create_indexed_both
class _NoIndex:
    _h = None


def _both(hip, max_occ=2, max_ref_occ=B.NO_CAP, **over):
    rs = B.Reads([S.KNOWN_Q, S.KNOWN_Q_MINUS, b"", b"ACGNACG"])
    a = dict(pool=rs.pool, q_off=rs.q_off, q_len=rs.q_len)
    a.update(over)
    return hip.Seeder.indexed_both(_NoIndex(), max_occ, max_ref_occ, a["pool"], a["q_off"], a["q_len"])


def test_the_both_strand_seeder_judges_its_other_arguments_before_the_index(hip):
    for kw in (dict(), dict(max_occ=1, max_ref_occ=1), dict(max_occ=B.NO_CAP)):
        with pytest.raises(RuntimeError, match="null index"):   # every check passed
            _both(hip, **kw)
    with pytest.raises(RuntimeError, match="max_occ must be at least 1"):
        _both(hip, max_occ=0)
    with pytest.raises(RuntimeError, match="max_ref_occ must be at least 1"):
        _both(hip, max_ref_occ=0)
    q_len = np.array([10, (1 << 31) - 16, 0, 7], np.uint32)
    with pytest.raises(RuntimeError, match=rf"read 1: the read \({(1 << 31) - 16} bytes\) must be shorter than 2\^31 - 16 bytes"):
        _both(hip, q_len=q_len)
    with pytest.raises(ValueError, match="one entry per problem"):
        _both(hip, q_len=q_len[:2])
    z = np.zeros(0, np.uint32)
    with pytest.raises(RuntimeError, match=r"a both-strand seeding batch must hold between 1 and 2\^27 reads"):
        hip.Seeder.indexed_both(_NoIndex(), 1, 1, np.zeros(4, np.uint8), z, z)
    L = hip.lib()
    one = np.zeros(2, np.uint64)
    assert not L.ba_seeding_create_indexed_both(None, 1, 1, one.ctypes.data, one.ctypes.data, one.ctypes.data, (1 << 27) + 1)   # (the count is judged first)
    assert re.search(r"between 1 and 2\^27 reads", hip.last_error())
    for k in range(3):
        args = [one.ctypes.data] * 3
        args[k] = None
        assert not L.ba_seeding_create_indexed_both(None, 1, 1, *args, 1) and "null argument" in hip.last_error(), k


def test_null_handles_are_refused(hip):
    L = hip.lib()
    assert L.ba_seeding_reload_indexed_both(None, None, None, None, 0) != 0 and "null batch" in hip.last_error()
    assert L.ba_seeding_problems(None, None, None) != 0 and "null batch" in hip.last_error()


def test_the_messages_of_mixed_use_name_the_other_call():
    """(Each needs a handle to be provoked: tests/test_gpu_index_both.py does that. Here: the texts are in the host source.)"""
    host = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_host.cpp")).read()
    for text in ("ba_seeding_create_indexed: the index is canonical and holds both strands; call ba_seeding_create_indexed_both",
                 "ba_seeding_create_indexed_both: the index is not canonical (ba_ref_index_create_canonical makes one); call ba_seeding_create_indexed",
                 "ba_seeding_reload: the seeder takes its reads on both strands at once; call ba_seeding_reload_indexed_both",
                 "ba_seeding_reload_indexed: the seeder takes its reads on both strands at once; call ba_seeding_reload_indexed_both",
                 "ba_seeding_reload_indexed_both: the seeder takes one strand per problem; call %s"):
        assert text in host, text


def test_the_release_library_reads_no_environment_variable_in_the_new_calls():
    """(The both-strand seeder is loaded and run by the seeding section's code, so both sections that hold a part of it are read whole.)"""
    host = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_host.cpp")).read()
    for first, last in (("// ------------------------------------------------------------------ minimizer seeding (ba_seeding_*)",
                         "// ------------------------------------------------------------------ read-level selection (ba_select_*)"),
                        ("// ------------------------------------------------------------------ the reference index (ba_ref_index_*, ba_seeding_*_indexed)",
                         "// Candidate windows for chain batches")):
        a, b = host.index(first), host.index(last)
        assert a < b and "getenv" not in host[a:b], first
    a = host.index("both strands at once (ba_seeding_*_indexed_both)")
    assert host.index("the reference index (ba_ref_index_*, ba_seeding_*_indexed)") < a < host.index("// Candidate windows for chain batches")


# ------------------------------------------------------------------ the kernels
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_new_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_index_both.hip"), "-o", str(tmp_path / "ba_index_both.o")], capture_output=True, text=True)
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
    assert len(scratch) == 6 and set(scratch.values()) == {0}, scratch   # every kernel of the unit, a count and an emit pass each
    for k in ("k_both_index_sketch", "k_both_read_sketch", "k_both_lookup"):
        assert [v for f, v in scratch.items() if k in f] == [0, 0], (k, scratch)


def test_kernel_hash_makefile_and_launch_header_list_the_new_unit():
    from tools import kernel_hash
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    assert "ba_index_both.hip" in kernel_hash.FILES
    assert re.search(r"^XOBJS := .*\$\(OBJ\)/ba_index_both\.o", mk, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/ba_index_both\.o: ba_index_both\.hip \$\(HDRS\)\n\t@mkdir -p \$\(OBJ\)\n\t\$\(HIPCC\) --offload-arch=\$\(ARCH\) \$\(CXXFLAGS\) -c ", mk, flags=re.M)
    launch = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_launch.h")).read()
    for f in ("ba_launch_both_index_sketch", "ba_launch_both_read_sketch", "ba_launch_both_lookup"):
        assert f in launch


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_sketch_kernels_keep_their_resources(tmp_path):
    """The plain and the canonical sketches are one loop (ba_seed_device.hpp). What the older paths' kernels must not pay for the newer
    ones is stated as what the compiler reports for all eight: no scratch, 8 waves per SIMD, and the LDS of their own staging area -- 4
    waves of 1728 bytes, and of 1856 with the canonical k-mers' strand bytes. The figures are those of the kernels before they shared."""
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    units = ("ba_seeding", "ba_index", "ba_index_both")
    runs = [subprocess.Popen(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                              "-c", os.path.join(csrc, u + ".hip"), "-o", str(tmp_path / (u + ".o"))], stderr=subprocess.PIPE, text=True) for u in units]
    figures = {}
    for u, r in zip(units, runs):
        err = r.communicate()[1]
        assert r.returncode == 0, err
        name = None
        for line in err.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                figures[name] = {}
            m = re.search(r"(ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
            if m and name:
                figures[name][m.group(1).split(" [")[0]] = int(m.group(2))
    lds = {"k_seeding_sketch": 6912, "k_index_sketch": 6912, "k_both_index_sketch": 7424, "k_both_read_sketch": 7424}
    for kernel, size in lds.items():
        got = [v for f, v in figures.items() if re.search(rf"\d{kernel}ILb[01]E", f)]
        assert got == [dict(ScratchSize=0, Occupancy=8, **{"LDS Size": size})] * 2, (kernel, got)   # the count pass and the emit pass
