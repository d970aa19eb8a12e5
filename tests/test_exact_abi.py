"""Exact scores and the accuracy summary without a GPU: the C calls are exported by both libraries and declared, struct BaExact is 16 bytes,
ba_accuracy_summary equals a numpy computation of every field, null arguments and over-long pairs are refused with a message, the kernel
hash covers the new sources, and the tests' own full-matrix DP agrees with tests/gotoh.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from block_aligner_amd import scores as S
from tests import exact_dp, gotoh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_batch_exact", "ba_sized_batch_exact", "ba_multibatch_exact", "ba_batch_exact_ms", "ba_extend_batch_exact", "ba_accuracy_summary",
         "ba_exact_check_lengths")
FAILED = 1 | 2 | 4 | 8 | 16 | 32 | 128   # overflow, lost and watchdog bits
CALLER = r"""
#include "block_aligner_hip.h"
typedef char exact_is_16_bytes[sizeof(struct BaExact) == 16 ? 1 : -1];
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, BaExtendBatch* e, const uint32_t* which) {
    struct BaExact rec[4], left[4], right[4];
    struct BaAccuracy acc;
    int32_t score[4] = {0, 0, 0, 0};
    uint32_t idx[4] = {0, 0, 0, 0};
    float ms; uint64_t cells;
    int rc = ba_batch_exact(b, BA_EXACT_GLOBAL, -1, which, 4, rec);
    rc |= ba_sized_batch_exact(s, BA_EXACT_EXTEND, 50, NULL, 0, rec);
    rc |= ba_multibatch_exact(m, BA_EXACT_EXTEND, -1, which, 4, rec);
    rc |= ba_batch_exact_ms(b, &ms, &cells);
    rc |= ba_extend_batch_exact(e, -1, which, 4, left, right, score);
    rc |= ba_exact_check_lengths(idx, idx, 4);
    rc |= ba_accuracy_summary(score, idx, idx, idx, rec, 4, &acc);
    return rc + (int)acc.wrong + (int)acc.mean_rel_error + acc.min_diff;
}
"""


def test_exact_symbols_are_exported(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_exact_calls_are_declared(tmp_path):
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


def test_exact_record_is_16_bytes(hip):
    assert ctypes.sizeof(hip.ExactC) == 16 and hip.EXACT_DTYPE.itemsize == 16
    assert [hip.EXACT_DTYPE.fields[k][1] for k in ("score", "query_idx", "reference_idx", "rows")] == [0, 4, 8, 12]
    assert (hip.EXACT_GLOBAL, hip.EXACT_EXTEND) == (0, 1)


def numpy_summary(score, qi, ri, status, ex_score, ex_qi, ex_ri):
    score, ex_score, qi, ri, status, ex_qi, ex_ri = (np.asarray(a, np.int64) for a in (score, ex_score, qi, ri, status, ex_qi, ex_ri))
    ok = (status & FAILED) == 0
    diff = (ex_score - score)[ok]
    wrong = diff != 0
    rel = diff[wrong & (ex_score[ok] != 0)] / np.abs(ex_score[ok][wrong & (ex_score[ok] != 0)])
    return dict(n=len(score), compared=int(ok.sum()), skipped=int((~ok).sum()), wrong=int(wrong.sum()), below=int((diff > 0).sum()),
                above=int((diff < 0).sum()), diff_end=int(((qi != ex_qi) | (ri != ex_ri))[ok].sum()),
                mean_rel_error=float(rel.mean()) if rel.size else 0.0, min_diff=int(diff[wrong].min()) if wrong.any() else 0,
                max_diff=int(diff[wrong].max()) if wrong.any() else 0)


SUMMARY_CASES = {
    # score, query_idx, reference_idx, status, exact score, exact query_idx, exact reference_idx
    "all_correct": ([10, -3, 0, 77], [5, 6, 0, 9], [5, 7, 0, 9], [0, 0, 0, 0], [10, -3, 0, 77], [5, 6, 0, 9], [5, 7, 0, 9]),
    "some_below": ([10, 40, 90, 77, -8], [5, 6, 7, 9, 2], [5, 7, 7, 9, 2], [0, 0, 0, 0, 0], [10, 50, 100, 77, -4], [5, 8, 7, 9, 2], [5, 7, 9, 9, 2]),
    "one_above": ([10, 55, 90], [5, 6, 7], [5, 7, 7], [0, 0, 0], [10, 50, 100], [5, 6, 7], [5, 7, 7]),
    "failed_is_skipped": ([10, 1, 90, 3, 5], [5, 6, 7, 1, 1], [5, 7, 7, 1, 1], [0, 4, 0, 16, 64], [10, 50, 100, 30, 5], [5, 6, 7, 1, 1], [5, 7, 8, 1, 2]),
    "exact_zero_among_wrong": ([-6, -2, 12], [1, 2, 3], [1, 2, 3], [0, 0, 0], [0, 0, 16], [0, 0, 3], [0, 0, 3]),
    "only_exact_zero_wrong": ([-6, 4], [1, 2], [1, 2], [0, 0], [0, 4], [0, 2], [0, 2]),
    "n_zero": ([], [], [], [], [], [], []),
}


@pytest.mark.parametrize("case", sorted(SUMMARY_CASES))
def test_accuracy_summary_equals_numpy(hip, case):
    score, qi, ri, status, es, eq, er = SUMMARY_CASES[case]
    rec = np.zeros(len(score), hip.EXACT_DTYPE)
    rec["score"], rec["query_idx"], rec["reference_idx"] = es, eq, er
    got = hip.accuracy_summary(np.array(score, np.int32), rec, np.array(qi, np.uint32), np.array(ri, np.uint32), np.array(status, np.uint32))
    want = numpy_summary(score, qi, ri, status, es, eq, er)
    assert {k: got[k] for k in want if k != "mean_rel_error"} == {k: want[k] for k in want if k != "mean_rel_error"}
    assert got["mean_rel_error"] == pytest.approx(want["mean_rel_error"], rel=1e-12, abs=0)
    # the same through a dict of arrays, as _Batch.exact() returns them
    again = hip.accuracy_summary(score, dict(score=es, query_idx=eq, reference_idx=er, rows=np.zeros(len(es))), qi, ri, status)
    assert again == got


def test_null_arguments_are_refused(hip):
    L = hip.lib()
    rec = np.zeros(2, hip.EXACT_DTYPE)
    for f in (L.ba_batch_exact, L.ba_sized_batch_exact, L.ba_multibatch_exact):
        assert f(None, 0, -1, None, 0, rec.ctypes.data) != 0
        assert "null batch" in hip.last_error()
        assert f(None, 0, -1, None, 0, None) != 0 and hip.last_error()
    ms, cells = ctypes.c_float(), ctypes.c_uint64()
    assert L.ba_batch_exact_ms(None, ctypes.byref(ms), ctypes.byref(cells)) != 0 and "null batch" in hip.last_error()
    sc = np.zeros(2, np.int32)
    assert L.ba_extend_batch_exact(None, -1, None, 0, rec.ctypes.data, rec.ctypes.data, sc.ctypes.data) != 0 and "null batch" in hip.last_error()
    assert L.ba_accuracy_summary(sc.ctypes.data, None, None, None, rec.ctypes.data, 2, None) != 0 and "out" in hip.last_error()
    out = hip.AccuracyC()
    assert L.ba_accuracy_summary(None, None, None, None, rec.ctypes.data, 2, ctypes.byref(out)) != 0 and "null" in hip.last_error()


def test_length_guard_names_the_pair(hip):
    """(|q| + |r|) * 128 must stay above the minus-infinity sentinel -2^30: |q| + |r| <= 2^23 - 1. Lengths only: nothing is allocated."""
    hip.exact_check_lengths([10, 1 << 22, 0], [10, (1 << 22) - 1, (1 << 23) - 1])
    with pytest.raises(RuntimeError, match=r"pair 2 .*too long"):
        hip.exact_check_lengths([10, 5, 1 << 22], [10, 5, 1 << 22])
    with pytest.raises(RuntimeError, match=r"pair 0 "):
        hip.exact_check_lengths([0xffffffff], [0xffffffff])


def test_kernel_hash_lists_the_exact_sources():
    from tools import kernel_hash
    assert "ba_exact.h" in kernel_hash.FILES and "ba_exact.hip" in kernel_hash.FILES


def _random_pairs(rng, alphabet, n, lower=False):
    out = []
    for _ in range(n):
        a = alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 70)))]
        b = alphabet[rng.integers(0, len(alphabet), int(rng.integers(0, 70)))]
        q, r = a.tobytes(), b.tobytes()
        out.append((q.lower(), r) if lower and len(out) % 3 == 0 else (q, r))
    return out


@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_exact_dp_equals_gotoh(kind):
    rng = np.random.default_rng({"nuc": 11, "aa": 12, "bytes": 13}[kind])
    if kind == "nuc":
        m, gaps, pairs = S.NucMatrix.new_simple(2, -3), (-5, -1), _random_pairs(rng, np.frombuffer(b"ACGT", np.uint8), 40, lower=True)
    elif kind == "aa":
        m, gaps, pairs = S.static_matrix("BLOSUM62"), (-11, -1), _random_pairs(rng, np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), 40, lower=True)
    else:
        m, gaps, pairs = S.ByteMatrix.new_simple(3, -2), (-4, -2), _random_pairs(rng, np.arange(250, 256, dtype=np.uint8), 40)
    pairs += [(b"", b""), (b"", pairs[0][1] or b"\xfa"), (pairs[1][0] or b"\xfa", b"")]
    for q, r in pairs:
        H = exact_dp.full_matrix(q, r, m, gaps)
        assert H.shape == (len(q) + 1, len(r) + 1) and H[0, 0] == 0
        assert int(H[-1, -1]) == gotoh.global_score(q, r, m, gaps), (q, r)
        assert exact_dp.exact_global(q, r, m, gaps) == (int(H[-1, -1]), len(q), len(r), len(q) + 1)
        s, i, j, rows = exact_dp.exact_extend(q, r, m, gaps)
        assert s == int(H.max()) >= 0 and int(H[i, j]) == s and rows == len(q) + 1
        assert (i, j) == tuple(int(x) for x in np.argwhere(H == s)[0])      # the smallest i, then the smallest j
        for x in (0, 5, 20):
            sx, ix, jx, rx = exact_dp.exact_extend(q, r, m, gaps, x)
            assert 0 <= sx <= s and int(H[ix, jx]) == sx and ix < rx <= len(q) + 1
            assert sx == int(H[:rx].max())
