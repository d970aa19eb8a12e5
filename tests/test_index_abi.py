"""The reference index without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, every argument rejection
is reported before a device is needed, ba_chain_windows (host only) equals the model of tests/index_ref.py, and the hand-written kernels
compile for gfx950 without scratch. ba_seeding_create_indexed looks at its index last, so its other arguments are judged here with a null
index; the two crosswise reload refusals need a seeder and are in tests/test_gpu_index.py::test_lifecycle."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import index_ref as X, seeding_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_ref_index_create", "ba_ref_index_counts", "ba_ref_index_entries", "ba_ref_index_times", "ba_ref_index_destroy",
         "ba_seeding_create_indexed", "ba_seeding_reload_indexed", "ba_chain_windows")
CALLER = r"""
#include "block_aligner_hip.h"
int use(const uint8_t* ref, const uint8_t* pool, const uint64_t* off, const uint32_t* len, const uint8_t* strand) {
    BaRefIndex* x = ba_ref_index_create(15, 10, ref, 1000);
    uint64_t n, ref_len, first[2], r_off[1]; uint32_t k, w, run, code[8], pos[8], q[8], r[8], l[8], r_len[1], r_anchor[8];
    float a, b, c, ms = 0.0f;
    BaSeeding* s;
    int rc = ba_ref_index_counts(x, &n, &k, &w, &ref_len, &run);
    rc |= ba_ref_index_counts(x, NULL, NULL, NULL, NULL, NULL);
    rc |= ba_ref_index_entries(x, code, pos);
    rc |= ba_ref_index_times(x, &a, &b, &c);
    s = ba_seeding_create_indexed(x, 64, 0xffffffffu, pool, off, len, strand, 1);
    ba_ref_index_destroy(x);
    rc |= ba_seeding_reload_indexed(s, pool, off, len, NULL, 1);
    rc |= ba_seeding_run(s, &ms);
    rc |= ba_seeding_results(s, first, q, r, l);
    rc |= ba_chain_windows(len, off, len, first, q, r, l, 1, 64, r_off, r_len, r_anchor);
    ba_seeding_destroy(s);
    return rc;
}
"""


def test_index_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_index_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _no_device(hip):
    try:
        return hip.device_count() < 1
    except Exception:
        return True


def _accepted(hip, k, w, ref):
    """The arguments pass every check: without a device they get as far as the device."""
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            hip.RefIndex(k, w, ref)
    else:
        hip.RefIndex(k, w, ref).close()


def test_valid_index_arguments_pass_every_check(hip):
    _accepted(hip, 5, 4, S.KNOWN_R)
    for k, w in ((4, 1), (16, 64)):   # the limits of the parameters
        _accepted(hip, k, w, S.KNOWN_R)
    _accepted(hip, 15, 10, b"ACGT")   # shorter than k: legal, no entries
    _accepted(hip, 15, 10, b"")


@pytest.mark.parametrize("k, w, message", [(3, 4, r"k must be between 4 and 16 \(it is 3\)"), (17, 4, r"k must be between 4 and 16 \(it is 17\)"),
                                           (5, 0, r"w must be between 1 and 64 \(it is 0\)"), (5, 65, r"w must be between 1 and 64 \(it is 65\)")])
def test_index_rejects_parameters_out_of_range(hip, k, w, message):
    with pytest.raises(RuntimeError, match=message):
        hip.RefIndex(k, w, S.KNOWN_R)


def test_index_rejects_a_null_reference_and_one_of_2_31_minus_16_bytes(hip):
    """(Only the length is read before the rejection: no such reference exists here.)"""
    L = hip.lib()
    one = np.zeros(8, np.uint8)
    assert not L.ba_ref_index_create(5, 4, None, 8) and "null argument" in hip.last_error()
    assert not L.ba_ref_index_create(5, 4, None, 0) and "null argument" in hip.last_error()
    for n in ((1 << 31) - 16, 1 << 31, 1 << 40):
        assert not L.ba_ref_index_create(5, 4, one.ctypes.data, n)
        assert re.search(rf"the reference \({n} bytes\) must be shorter than 2\^31 - 16 bytes", hip.last_error())


class _NoIndex:
    _h = None


def _indexed(hip, max_occ=2, max_ref_occ=X.NO_CAP, **over):
    rs = X.known_reads()
    a = dict(pool=rs.pool, q_off=rs.q_off, q_len=rs.q_len, strand=rs.strand)
    a.update(over)
    return hip.Seeder.indexed(_NoIndex(), max_occ, max_ref_occ, a["pool"], a["q_off"], a["q_len"], a["strand"])


def test_indexed_seeder_judges_its_other_arguments_before_the_index(hip):
    for kw in (dict(), dict(strand=None), dict(max_occ=1, max_ref_occ=1), dict(max_occ=X.NO_CAP)):
        with pytest.raises(RuntimeError, match="null index"):   # every check passed
            _indexed(hip, **kw)
    with pytest.raises(RuntimeError, match="max_occ must be at least 1"):
        _indexed(hip, max_occ=0)
    with pytest.raises(RuntimeError, match="max_ref_occ must be at least 1"):
        _indexed(hip, max_ref_occ=0)
    n = len(X.known_reads())
    with pytest.raises(RuntimeError, match="problem 2: strand must be 0 or 1"):
        _indexed(hip, strand=np.array([0, 1, 2] + [0] * (n - 3), np.uint8))
    q_len = X.known_reads().q_len.copy()
    q_len[1] = (1 << 31) - 16
    with pytest.raises(RuntimeError, match=r"problem 1: the sequences .* must be shorter than 2\^31 - 16 bytes"):
        _indexed(hip, q_len=q_len)
    with pytest.raises(ValueError, match="one entry per problem"):
        _indexed(hip, q_len=q_len[:2])
    with pytest.raises(ValueError, match="one entry per problem"):
        _indexed(hip, strand=np.zeros(2, np.uint8))
    z = np.zeros(0, np.uint32)
    with pytest.raises(RuntimeError, match="between 1 and 2\\^28 problems"):
        hip.Seeder.indexed(_NoIndex(), 1, 1, np.zeros(4, np.uint8), z, z)


def test_null_handles_and_null_arguments_are_refused(hip):
    L = hip.lib()
    assert L.ba_ref_index_counts(None, *([None] * 5)) != 0 and "null index" in hip.last_error()
    assert L.ba_ref_index_entries(None, None, None) != 0 and "null index" in hip.last_error()
    assert L.ba_ref_index_times(None, None, None, None) != 0 and "null index" in hip.last_error()
    L.ba_ref_index_destroy(None)
    assert L.ba_seeding_reload_indexed(None, *([None] * 4), 0) != 0 and "null batch" in hip.last_error()
    one = np.zeros(2, np.uint64)
    for k in range(3):
        args = [one.ctypes.data] * 3
        args[k] = None
        assert not L.ba_seeding_create_indexed(None, 1, 1, *args, None, 1) and "null argument" in hip.last_error(), k
    out = [np.zeros(2, np.uint64) for _ in range(3)]
    for k in range(10):   # every array of ba_chain_windows, outputs included
        args = [one.ctypes.data] * 7 + [1, 10] + [o.ctypes.data for o in out]
        args[k if k < 7 else k + 2] = None
        assert L.ba_chain_windows(*args) != 0 and "null argument" in hip.last_error(), k


def _random_chains(rng, n):
    """n chains over reads of 50 .. 400 bases against references of 300 .. 5000, colinear anchors anywhere inside them."""
    q_len, r_len, r_off, first, qa, ra, ln = [], [], [], [0], [], [], []
    for _ in range(n):
        ql, rl = int(rng.integers(50, 401)), int(rng.integers(300, 5001))
        K = int(rng.integers(1, 6))
        L = rng.integers(4, 9, K)
        q_at = np.sort(rng.choice(ql // 10, K, replace=False)) * 10      # (steps of 10: anchors of at most 8 columns stay disjoint)
        r_at = np.sort(rng.choice(rl // 10, K, replace=False)) * 10
        q_len.append(ql); r_len.append(rl); r_off.append(int(rng.integers(0, 1 << 33)))
        qa += q_at.tolist(); ra += r_at.tolist(); ln += L.tolist()
        first.append(len(qa))
    return q_len, r_off, r_len, first, qa, ra, ln


@pytest.mark.parametrize("margin", [0, 1, 64, 100000, 0xffffffff])
def test_chain_windows_equal_the_model(hip, margin):
    rng = np.random.default_rng(5 + margin % 1000)
    a = _random_chains(rng, 200)
    got, want = hip.chain_windows(*a, margin), X.chain_windows(*a, margin)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    r_off_w, r_len_w, r_anchor_w, shift = got
    for c in range(200):   # a valid input of ba_chain_batch_create: every anchor inside the window, which is inside the reference
        lo, hi = a[3][c], a[3][c + 1]
        assert all(int(r_anchor_w[i]) + a[6][i] <= int(r_len_w[c]) for i in range(lo, hi))
        assert int(shift[c]) + int(r_len_w[c]) <= a[2][c] and int(r_off_w[c]) == a[1][c] + int(shift[c])


def test_chain_windows_by_hand_and_its_rejections(hip):
    r_off_w, r_len_w, r_anchor_w, shift = hip.chain_windows([100] * 4, [5000] * 4, [1000] * 4, [0, 2, 4, 6, 7], [20, 40, 10, 60, 30, 50, 0],
                                                            [5, 26, 900, 960, 500, 520, 300], [10, 10, 10, 20, 10, 30, 100], 10)
    assert shift.tolist() == [0, 880, 460, 290] and r_off_w.tolist() == [5000, 5880, 5460, 5290]   # tests/test_index_ref.py::test_windows_by_hand
    assert r_len_w.tolist() == [96, 120, 120, 120] and r_anchor_w.tolist() == [5, 26, 20, 80, 40, 60, 10]
    with pytest.raises(RuntimeError, match="chain 1 has no anchors"):
        hip.chain_windows([100, 100], [0, 0], [1000, 1000], [0, 1, 1], [0], [0], [10], 10)
    with pytest.raises(RuntimeError, match="chain 0: anchor 1 ends outside its sequences"):
        hip.chain_windows([100], [0], [1000], [0, 2], [0, 95], [0, 200], [10, 10], 10)
    with pytest.raises(RuntimeError, match="chain 2: anchor 0 ends outside its sequences"):
        hip.chain_windows([100] * 3, [0] * 3, [1000] * 3, [0, 1, 2, 3], [0, 0, 0], [0, 0, 995], [10, 10, 10], 10)
    with pytest.raises(ValueError, match="one entry per chain"):
        hip.chain_windows([100], [0, 0], [1000], [0, 1], [0], [0], [10], 10)
    with pytest.raises(ValueError, match="one entry per anchor"):
        hip.chain_windows([100], [0], [1000], [0, 2], [0], [0], [10], 10)
    none = hip.chain_windows(np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32), [0], [], [], [], 10)
    assert [len(x) for x in none] == [0, 0, 0, 0]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_index_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_index.hip"), "-o", str(tmp_path / "ba_index.o")], capture_output=True, text=True)
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
    assert len(scratch) == 6 and set(scratch.values()) == {0}, scratch   # every kernel of the unit, and no library kernel among them
    for k, passes in (("k_index_sketch", 2), ("k_index_table", 1), ("k_index_lookup", 2), ("k_index_hit_sort", 1)):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0] * passes, (k, scratch)


def test_kernel_hash_makefile_and_launch_header_list_the_index_sources():
    from tools import kernel_hash
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    for f in ("ba_index.hip", "ba_index_sort.hip", "ba_index.h", "ba_seed_device.hpp"):
        assert f in kernel_hash.FILES, f
    for obj in ("ba_index", "ba_index_sort"):
        assert re.search(rf"^XOBJS := .*\$\(OBJ\)/{obj}\.o", mk, flags=re.M), obj
    for h in ("ba_index.h", "ba_seed_device.hpp"):
        assert re.search(rf"^HDRS := .*\b{re.escape(h)}\b", mk, flags=re.M), h
    launch = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_launch.h")).read()
    for f in ("ba_launch_index_sketch", "ba_launch_index_sort", "ba_launch_index_table", "ba_launch_index_lookup", "ba_launch_index_hit_sort"):
        assert f in launch
    span = int(re.search(r"INDEX_SPAN = (\d+)", open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_index.h")).read()).group(1))
    assert span == X.SPAN and span % 64 == 0   # what the seam tests straddle
