"""Optimal paths in the batch's own mode without a GPU: the C calls are exported by both libraries and declared, a C caller compiles,
struct BaExactPath is 24 bytes, null arguments are refused with a message, the Python surface exists and the length guard of profile
pairs counts (|q| + 1) * |r|."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_batch_exact_paths", "ba_sized_batch_exact_paths", "ba_multibatch_exact_paths", "ba_extend_batch_exact_paths", "ba_batch_exact_paths_ms",
         "ba_exact_paths_check_lengths_profile")
CALLER = r"""
#include "block_aligner_hip.h"
typedef char path_is_24_bytes[sizeof(struct BaExactPath) == 24 ? 1 : -1];
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, BaExtendBatch* e, const uint32_t* which) {
    struct BaExactPath rec[4];
    struct BaExact left[4], right[4];
    uint64_t off[5], cells;
    uint32_t runs[64], len[4] = {1, 1, 1, 1};
    float ms;
    int rc = ba_batch_exact_paths(b, BA_EXACT_GLOBAL, -1, which, 4, rec, off, NULL, 0);
    rc |= ba_batch_exact_paths(b, BA_EXACT_EXTEND | BA_EXACT_OWN_MODE, 30, NULL, 0, rec, off, runs, 64);
    rc |= ba_sized_batch_exact_paths(s, BA_EXACT_EXTEND, 50, NULL, 0, rec, off, runs, 64);
    rc |= ba_multibatch_exact_paths(m, BA_EXACT_GLOBAL, -1, which, 4, rec, off, runs, 64);
    rc |= ba_extend_batch_exact_paths(e, -1, which, 4, rec, left, right, off, runs, 64);
    rc |= ba_extend_batch_exact_paths(e, -1, which, 4, rec, NULL, NULL, off, NULL, 0);
    rc |= ba_batch_exact_paths_ms(b, &ms, &cells);
    rc |= ba_exact_paths_check_lengths_profile(len, len, 4);
    return rc + rec[0].score + (int)(rec[0].q_start + rec[0].r_start + rec[0].q_end + rec[0].r_end + rec[0].rows);
}
"""


def test_path_symbols_are_exported(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_path_calls_are_declared(tmp_path):
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


def test_path_record_is_24_bytes(hip):
    assert ctypes.sizeof(hip.ExactPathC) == 24 and hip.EXACT_PATH_DTYPE.itemsize == 24
    assert [hip.EXACT_PATH_DTYPE.fields[k][1] for k in ("score", "q_start", "r_start", "q_end", "r_end", "rows")] == [0, 4, 8, 12, 16, 20]


def test_null_arguments_are_refused(hip):
    L = hip.lib()
    rec, off = np.zeros(2, hip.EXACT_PATH_DTYPE), np.zeros(3, np.uint64)
    for f in (L.ba_batch_exact_paths, L.ba_sized_batch_exact_paths, L.ba_multibatch_exact_paths):
        assert f(None, 0, -1, None, 0, rec.ctypes.data, off.ctypes.data, None, 0) != 0
        assert "null batch" in hip.last_error()
        assert f(None, 0, -1, None, 0, None, off.ctypes.data, None, 0) != 0
        assert "null argument: out" in hip.last_error()
        assert f(None, 0, -1, None, 0, rec.ctypes.data, None, None, 0) != 0
        assert "null argument: run_off" in hip.last_error()
    f = L.ba_extend_batch_exact_paths
    assert f(None, -1, None, 0, rec.ctypes.data, None, None, off.ctypes.data, None, 0) != 0 and "null batch" in hip.last_error()
    assert f(None, -1, None, 0, None, None, None, off.ctypes.data, None, 0) != 0 and "null argument: out" in hip.last_error()
    assert f(None, -1, None, 0, rec.ctypes.data, None, None, None, None, 0) != 0 and "null argument: run_off" in hip.last_error()
    assert L.ba_batch_exact_paths_ms(None, None, None) != 0 and "null batch" in hip.last_error()


def test_python_surface(hip):
    for cls in (hip.BatchAligner, hip.SizedBatchAligner, hip.MultiBatchAligner, hip.ProfileBatchAligner, hip.ExtendBatchAligner):
        assert callable(getattr(cls, "exact_paths")), cls
    assert callable(hip.BatchAligner.exact_paths_ms)
    assert hip.EXACT_PATH_DTYPE.names == ("score", "q_start", "r_start", "q_end", "r_end", "rows")


def test_profile_pairs_count_row_zero(hip):
    """(|q| + 1) * |r| against EXACT_TRACE_MAX_CELLS = 2^31: |q| = 65535, |r| = 32768 is the largest profile pair of that width."""
    hip.exact_trace_check_lengths([65535], [32768])
    hip.exact_paths_check_lengths_profile([65535], [32768])
    with pytest.raises(RuntimeError, match=r"pair 1 .*profile.*too large for a traced matrix"):
        hip.exact_paths_check_lengths_profile([10, 65535], [10, 32768 + 1])
    with pytest.raises(RuntimeError, match=r"pair 0 .*\(\|q\| \+ 1\) \* \|r\|"):
        hip.exact_paths_check_lengths_profile([65536], [32768])
