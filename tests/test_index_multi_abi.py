"""Several sequences in one index without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, every
refusal arrives with its message before a device is needed, ba_chain_windows_seqs and ba_ref_locate (host only) equal the models of
tests/index_multi_ref.py, and the bounded fill is a unit of its own beside the unchanged one."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chaining_ref as C, index_multi_ref as M, seeding_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_ref_index_create_multi", "ba_ref_index_sequences", "ba_chaining_create_bounded", "ba_chain_windows_seqs", "ba_ref_locate")
CALLER = r"""
#include "block_aligner_hip.h"
int use(const uint8_t* pool, const uint64_t* off, const uint32_t* len, const struct BaChainingParams* P) {
    BaRefIndex* x = ba_ref_index_create_multi(15, 10, pool, off, len, 3);
    uint64_t n, start[4], first[2], r_off[1]; uint32_t q[8], r[8], l[8], r_len[1], r_anchor[8], seq[1], shift[1], a[1], b[1]; uint8_t crosses[1];
    BaSeeding* s = ba_seeding_create_indexed(x, 64, 0xffffffffu, pool, off, len, NULL, 1);
    BaChaining* c;
    int rc = ba_ref_index_sequences(x, &n, NULL);
    rc |= ba_ref_index_sequences(x, &n, start);
    rc |= ba_seeding_run(s, NULL);
    rc |= ba_seeding_results(s, first, q, r, l);
    c = ba_chaining_create_seeded(P, s);
    ba_chaining_destroy(c);
    c = ba_chaining_create_bounded(P, first, q, r, l, 1, start, 3);
    rc |= ba_chain_windows_seqs(len, first, q, r, l, 1, 64, off, len, 3, r_off, r_len, r_anchor, seq, shift);
    rc |= ba_ref_locate(len, 3, r, r, 1, seq, a, b, crosses);
    ba_chaining_destroy(c); ba_seeding_destroy(s); ba_ref_index_destroy(x);
    return rc;
}
"""
GOOD = (4, 1, 0, 64, 400, 60, 4, 24, 1)
LIMIT = 0x7fffffff - 16   # ba::SEEDING_MAX_LEN, the limit of ba_ref_index_create: the first total length that is refused


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


# ------------------------------------------------------------------ ba_ref_index_create_multi
def test_valid_sequences_pass_every_check(hip):
    _accepted(hip, lambda: hip.RefIndex.from_sequences(5, 4, [S.KNOWN_R, b"", S.KNOWN_R[:3]]))
    _accepted(hip, lambda: hip.RefIndex.from_sequences(16, 64, [b""]))
    pool = np.frombuffer(b"##" + S.KNOWN_R + b"#" + S.KNOWN_Q, np.uint8)   # apart, and not in order
    _accepted(hip, lambda: hip.RefIndex.from_sequences(5, 4, pool, [3 + len(S.KNOWN_R), 2, 0], [len(S.KNOWN_Q), len(S.KNOWN_R), 0]))
    _accepted(hip, lambda: hip.RefIndex.from_sequences(4, 1, np.zeros(8, np.uint8), np.zeros(1 << 20, np.uint64), np.zeros(1 << 20, np.uint32)))


def test_create_multi_refusals(hip):
    L = hip.lib()
    one = np.zeros(8, np.uint64)
    for k in range(3):
        args = [one.ctypes.data] * 3
        args[k] = None
        assert not L.ba_ref_index_create_multi(5, 4, *args, 1) and "null argument" in hip.last_error(), k
    for k, w, message in ((3, 4, r"k must be between 4 and 16 \(it is 3\)"), (5, 65, r"w must be between 1 and 64 \(it is 65\)")):
        with pytest.raises(RuntimeError, match=message):
            hip.RefIndex.from_sequences(k, w, [S.KNOWN_R])
    with pytest.raises(RuntimeError, match=r"between 1 and 2\^20 sequences \(it has 0\)"):
        hip.RefIndex.from_sequences(5, 4, [])
    n = (1 << 20) + 1
    with pytest.raises(RuntimeError, match=rf"between 1 and 2\^20 sequences \(it has {n}\)"):
        hip.RefIndex.from_sequences(5, 4, np.zeros(8, np.uint8), np.zeros(n, np.uint64), np.zeros(n, np.uint32))
    # the total length at the limit (only the lengths are read before the refusal: no such sequences exist here)
    lens = np.array([1 << 30, (1 << 30) - 17, 0], np.uint32)
    assert not L.ba_ref_index_create_multi(5, 4, one.ctypes.data, one.ctypes.data, lens.ctypes.data, 3)
    assert re.search(rf"the sequences \({LIMIT} bytes in all\) must be shorter than 2\^31 - 16 bytes", hip.last_error())
    lens = np.full(3, 0xffffffff, np.uint32)   # (the sum does not wrap)
    assert not L.ba_ref_index_create_multi(5, 4, one.ctypes.data, one.ctypes.data, lens.ctypes.data, 3)
    assert re.search(rf"the sequences \({3 * 0xffffffff} bytes in all\)", hip.last_error())
    with pytest.raises(ValueError, match="one entry per sequence"):
        hip.RefIndex.from_sequences(5, 4, np.zeros(8, np.uint8), [0, 1], [2])
    with pytest.raises(ValueError, match="ends beyond the pool"):
        hip.RefIndex.from_sequences(5, 4, np.zeros(8, np.uint8), [0, 4], [4, 5])
    assert L.ba_ref_index_sequences(None, None, None) != 0 and "null index" in hip.last_error()


# ------------------------------------------------------------------ ba_chaining_create_bounded
def _bounded(hip, start, problem=None, params=GOOD):
    q, r, L = problem or M.junction_problem()
    ps = C.ProblemSet([(q, r, L)])
    return hip.AnchorChainer(*params, *ps.args(), seq_start=start)


def test_valid_bounded_arguments_pass_every_check(hip):
    _accepted(hip, lambda: _bounded(hip, M.JUNCTION_START))
    _accepted(hip, lambda: _bounded(hip, [0, LIMIT - 1]))
    _accepted(hip, lambda: _bounded(hip, [0] * 5 + [3000] * 3))
    _accepted(hip, lambda: _bounded(hip, [0, 892, 960, 972, 3000]))   # anchors that end exactly at a junction


def test_bounded_refusals(hip):
    L = hip.lib()
    P = hip.ChainingParamsC(*GOOD)
    one = np.zeros(2, np.uint64)
    for k in range(5):
        args = [one.ctypes.data] * 4 + [1, one.ctypes.data, 1]
        args[k if k < 4 else 5] = None
        assert not L.ba_chaining_create_bounded(ctypes.byref(P), *args) and "null argument" in hip.last_error(), k
    assert not L.ba_chaining_create_bounded(None, *([one.ctypes.data] * 4), 1, one.ctypes.data, 1) and "null argument" in hip.last_error()
    big = np.zeros((1 << 20) + 2, np.uint64)
    for n in (0, (1 << 20) + 1):
        assert not L.ba_chaining_create_bounded(ctypes.byref(P), *([one.ctypes.data] * 4), 1, big.ctypes.data, n)
        assert re.search(rf"a sequence table must hold between 1 and 2\^20 sequences \(it has {n}\)", hip.last_error())
    with pytest.raises(RuntimeError, match=r"seq_start must start at 0 \(sequence 0 starts at 5\)"):
        _bounded(hip, [5, 3000])
    with pytest.raises(RuntimeError, match=r"sequence 1: seq_start must not decrease \(900 after 1000\)"):
        _bounded(hip, [0, 1000, 900, 3000])
    with pytest.raises(RuntimeError, match=rf"the sequences \({LIMIT} bytes in all\) must be shorter than 2\^31 - 16 bytes"):
        _bounded(hip, [0, LIMIT])
    with pytest.raises(ValueError, match="one entry per sequence and one more"):
        _bounded(hip, [])
    # ba_chaining_create's own checks still hold ...
    with pytest.raises(RuntimeError, match="lookback must be between 1 and 1024"):
        _bounded(hip, M.JUNCTION_START, params=GOOD[:3] + (0,) + GOOD[4:])
    with pytest.raises(RuntimeError, match="anchor_len must be at least 1"):
        _bounded(hip, M.JUNCTION_START, problem=([5], [5], [0]))
    # ... and an anchor that leaves its sequence is named: anchor 4 of the junction problem covers 960 .. 972
    with pytest.raises(RuntimeError, match=r"problem 0, anchor 4: the anchor covers reference 960 to 972 and leaves its sequence, which ends at 970"):
        _bounded(hip, [0, 970, 3000])
    with pytest.raises(RuntimeError, match=r"problem 0, anchor 11: .* leaves its sequence, which ends at 1105"):
        _bounded(hip, [0, 1000, 1105])   # beyond the last sequence's end
    with pytest.raises(RuntimeError, match=r"problem 0, anchor 0: .* leaves its sequence, which ends at 100"):
        _bounded(hip, [0, 50, 100, 100])   # an anchor behind everything


# ------------------------------------------------------------------ ba_chain_windows_seqs and ba_ref_locate
def _random_chains(rng, n, seq_len):
    """n chains of 1 .. 5 colinear anchors, each chain inside one non-empty sequence, some at its very first or last base."""
    start = [0] + np.cumsum(seq_len).tolist()
    full = [s for s in range(len(seq_len)) if seq_len[s] >= 60]
    q_len, first, qa, ra, ln = [], [0], [], [], []
    for c in range(n):
        s = full[int(rng.integers(0, len(full)))]
        ql, K = int(rng.integers(60, 401)), int(rng.integers(1, 6))
        L = rng.integers(4, 9, K)
        q_at = np.sort(rng.choice(ql // 10, K, replace=False)) * 10      # (steps of 10: anchors of at most 8 columns stay disjoint)
        r_at = np.sort(rng.choice(seq_len[s] // 10, K, replace=False)) * 10
        if c % 7 == 0:
            r_at[0] = 0
        if c % 7 == 1:
            r_at[-1] = seq_len[s] - int(L[-1])
        q_len.append(ql)
        qa += q_at.tolist(); ra += (r_at + start[s]).tolist(); ln += L.tolist()
        first.append(len(qa))
    return q_len, first, qa, ra, ln


SEQ_LEN = [700, 0, 60, 5000, 0, 0, 1, 300, 0]


@pytest.mark.parametrize("margin", [0, 1, 64, 100000, 0xffffffff])
def test_chain_windows_seqs_equal_the_model(hip, margin):
    rng = np.random.default_rng(9 + margin % 1000)
    seq_off = rng.permutation(len(SEQ_LEN)).astype(np.uint64) * np.uint64(1 << 33) + np.uint64(17)   # anywhere in a pool, in any order
    a = _random_chains(rng, 200, SEQ_LEN)
    got, want = hip.chain_windows_seqs(*a, margin, seq_off, SEQ_LEN), M.chain_windows_seqs(*a, margin, seq_off, SEQ_LEN)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    r_off_w, r_len_w, r_anchor_w, seq, shift = got
    for c in range(200):   # a valid input of ba_chain_batch_create: every anchor inside the window, which is inside its sequence
        lo, hi = a[1][c], a[1][c + 1]
        assert all(int(r_anchor_w[i]) + a[4][i] <= int(r_len_w[c]) for i in range(lo, hi))
        assert int(shift[c]) + int(r_len_w[c]) <= SEQ_LEN[int(seq[c])] and int(r_off_w[c]) == int(seq_off[int(seq[c])]) + int(shift[c])
    if margin >= 100000:   # larger than every sequence: the window is the sequence
        assert (shift == 0).all() and r_len_w.tolist() == [SEQ_LEN[int(s)] for s in seq]


def test_chain_windows_seqs_by_hand_and_its_refusals(hip):
    seq_len, seq_off = [1000, 0, 500], [7000, 0, 100]
    first, qa, ra, ln = [0, 1, 2, 4], [0, 90, 10, 40], [0, 990, 1010, 1040], [10, 10, 10, 10]
    r_off, r_len, r_anchor, seq, shift = hip.chain_windows_seqs([100] * 3, first, qa, ra, ln, 5, seq_off, seq_len)
    assert seq.tolist() == [0, 0, 2] and shift.tolist() == [0, 895, 0]   # tests/test_index_multi_ref.py::test_windows_and_locate_by_hand
    assert r_off.tolist() == [7000, 7895, 100] and r_len.tolist() == [105, 105, 105] and r_anchor.tolist() == [0, 95, 10, 40]
    with pytest.raises(RuntimeError, match="chain 1 has no anchors"):
        hip.chain_windows_seqs([100, 100], [0, 1, 1], [0], [0], [10], 10, seq_off, seq_len)
    with pytest.raises(RuntimeError, match="chain 0: anchor 0 ends outside its sequences"):
        hip.chain_windows_seqs([100], [0, 1], [0], [995], [10], 10, seq_off, seq_len)    # beyond E: over the junction at 1000
    with pytest.raises(RuntimeError, match="chain 0: anchor 1 ends outside its sequences"):
        hip.chain_windows_seqs([100], [0, 2], [0, 20], [980, 1000], [10, 10], 10, seq_off, seq_len)   # the chain's sequence is its first anchor's
    with pytest.raises(RuntimeError, match="chain 1: anchor 0 ends outside its sequences"):
        hip.chain_windows_seqs([100, 100], [0, 1, 2], [0, 95], [0, 0], [10, 10], 10, seq_off, seq_len)   # beyond q_len
    with pytest.raises(RuntimeError, match="chain 0: anchor 0 ends outside its sequences"):
        hip.chain_windows_seqs([100], [0, 1], [0], [1495], [10], 10, seq_off, seq_len)   # beyond the last sequence
    with pytest.raises(RuntimeError, match=r"between 1 and 2\^20 sequences \(it has 0\)"):
        hip.chain_windows_seqs([100], [0, 1], [0], [0], [10], 10, [], [])
    with pytest.raises(RuntimeError, match=rf"the sequences \({LIMIT} bytes in all\)"):
        hip.chain_windows_seqs([100], [0, 1], [0], [0], [10], 10, [0, 0], [LIMIT - 1, 1])
    with pytest.raises(ValueError, match="one entry per chain"):
        hip.chain_windows_seqs([100], [0, 1, 2], [0], [0], [10], 10, seq_off, seq_len)
    with pytest.raises(ValueError, match="one entry per anchor"):
        hip.chain_windows_seqs([100], [0, 2], [0], [0], [10], 10, seq_off, seq_len)
    with pytest.raises(ValueError, match="one entry per sequence"):
        hip.chain_windows_seqs([100], [0, 1], [0], [0], [10], 10, seq_off, seq_len[:2])
    L = hip.lib()
    one = np.zeros(2, np.uint64)
    for k in range(12):   # every array, outputs included
        args = [one.ctypes.data] * 5 + [1, 10] + [one.ctypes.data] * 2 + [1] + [one.ctypes.data] * 5
        args[k if k < 5 else k + 2 if k < 7 else k + 3] = None
        assert L.ba_chain_windows_seqs(*args) != 0 and "null argument" in hip.last_error(), k
    none = hip.chain_windows_seqs(np.zeros(0, np.uint32), [0], [], [], [], 10, seq_off, seq_len)
    assert [len(x) for x in none] == [0] * 5


def test_locate_equals_the_model(hip):
    rng = np.random.default_rng(15)
    total = sum(SEQ_LEN)
    a = rng.integers(0, total + 1, 500)
    b = np.minimum(a + rng.integers(0, 800, 500) * (rng.random(500) < 0.8), total)
    got, want = hip.locate(SEQ_LEN, a, b), M.locate(SEQ_LEN, a, b)
    assert got.keys() == want.keys()
    for key in want:
        assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
    assert got["crosses"].any() and not got["crosses"].all()
    assert all(SEQ_LEN[int(s)] > 0 for s in got["seq"])
    # trailing empty sequences, and nothing but empty ones
    assert hip.locate([10, 0, 0], [10], [10])["seq"].tolist() == [0] == M.locate([10, 0, 0], [10], [10])["seq"].tolist()
    z = hip.locate([0, 0], [0], [0])
    assert (z["seq"].tolist(), z["local_start"].tolist(), z["local_end"].tolist(), z["crosses"].tolist()) == ([0], [0], [0], [0])


def test_locate_by_hand_and_its_refusals(hip):
    seq_len = [1000, 0, 500]
    #           inside; ending exactly at the junction; one past it; empty at the junction; empty at the very end; the last base
    loc = hip.locate(seq_len, [0, 990, 990, 1000, 1500, 1499], [10, 1000, 1001, 1000, 1500, 1500])
    assert loc["seq"].tolist() == [0, 0, 0, 2, 2, 2]   # tests/test_index_multi_ref.py::test_windows_and_locate_by_hand
    assert loc["local_start"].tolist() == [0, 990, 990, 0, 500, 499] and loc["local_end"].tolist() == [10, 1000, 1001, 0, 500, 500]
    assert loc["crosses"].tolist() == [0, 0, 1, 0, 0, 0]
    with pytest.raises(RuntimeError, match=r"interval 1: 5 to 4 is not an interval of the index's 1500 bytes"):
        hip.locate(seq_len, [0, 5], [0, 4])
    with pytest.raises(RuntimeError, match=r"interval 0: 0 to 1501 is not an interval"):
        hip.locate(seq_len, [0], [1501])
    with pytest.raises(RuntimeError, match=r"interval 2: 1501 to 1501 is not an interval"):
        hip.locate(seq_len, [0, 0, 1501], [0, 0, 1501])
    with pytest.raises(RuntimeError, match=r"between 1 and 2\^20 sequences \(it has 0\)"):
        hip.locate([], [0], [0])
    with pytest.raises(RuntimeError, match=rf"the sequences \({LIMIT} bytes in all\)"):
        hip.locate([LIMIT], [0], [0])
    with pytest.raises(ValueError, match="one entry per interval"):
        hip.locate(seq_len, [0, 1], [0])
    L = hip.lib()
    one = np.zeros(2, np.uint64)
    for k in range(7):
        args = [one.ctypes.data, 1, one.ctypes.data, one.ctypes.data, 1] + [one.ctypes.data] * 4
        args[(0, 2, 3, 5, 6, 7, 8)[k]] = None
        assert L.ba_ref_locate(*args) != 0 and "null argument" in hip.last_error(), k
    assert [len(x) for x in hip.locate(seq_len, [], []).values()] == [0] * 4


# ------------------------------------------------------------------ the kernels
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_bounded_fill_is_a_unit_of_its_own_without_scratch(tmp_path):
    """ba_chaining.hip with BA_CHAINING_UNIT=1 holds the bounded fill and nothing else; the unit every other chainer runs (the default, pinned
    by tests/test_chaining_abi.py) does not hold it."""
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    names = {}
    for unit in (0, 1):
        r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                            f"-DBA_CHAINING_UNIT={unit}", "-c", os.path.join(csrc, "ba_chaining.hip"), "-o", str(tmp_path / f"unit{unit}.o")],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        scratch, name = {}, None
        for line in r.stderr.splitlines():
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and name:
                scratch[name] = int(m.group(1))
        assert set(scratch.values()) == {0}, scratch
        names[unit] = sorted(scratch)
    assert len(names[1]) == 1 and "k_chaining_fillILb1EE" in names[1][0], names
    assert len(names[0]) == 3 and [n for n in names[0] if "k_chaining_fill" in n] == [n for n in names[0] if "k_chaining_fillILb0EE" in n], names


def test_makefile_and_launch_header_list_the_bounded_unit():
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    assert re.search(r"^XOBJS := .*\$\(OBJ\)/ba_chaining_bounded\.o", mk, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/ba_chaining_bounded\.o: ba_chaining\.hip \$\(HDRS\)\n\t@mkdir -p \$\(OBJ\)\n\t.*-DBA_CHAINING_UNIT=1 ", mk, flags=re.M)
    launch = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "ba_launch.h")).read()
    assert "ba_launch_chaining_fill_bounded" in launch
