"""The exact-path calls without a GPU: exported by both libraries, declared in the header so that a C caller compiles, the traced length
limit accepts a pair at the limit and refuses one above it by name, and null arguments are refused with a message."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_batch_exact_cigars", "ba_sized_batch_exact_cigars", "ba_multibatch_exact_cigars", "ba_batch_exact_cigars_ms", "ba_exact_trace_check_lengths")
CALLER = r"""
#include "block_aligner_hip.h"
typedef char limit_is_below_2_gib_at_4_bits[BA_EXACT_TRACE_MAX_CELLS / 2 < (1ull << 31) ? 1 : -1];
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, const uint32_t* which) {
    struct BaExact rec[4];
    uint64_t off[5];
    uint32_t runs[64];
    uint32_t len[4] = {1, 2, 3, 4};
    float ms; uint64_t cells;
    int rc = ba_batch_exact_cigars(b, BA_EXACT_GLOBAL, -1, which, 4, rec, off, NULL, 0);
    rc |= ba_batch_exact_cigars(b, BA_EXACT_GLOBAL, -1, which, 4, rec, off, runs, 64);
    rc |= ba_sized_batch_exact_cigars(s, BA_EXACT_EXTEND, 50, NULL, 0, rec, off, runs, 64);
    rc |= ba_multibatch_exact_cigars(m, BA_EXACT_EXTEND, -1, which, 4, rec, off, runs, 64);
    rc |= ba_batch_exact_cigars_ms(b, &ms, &cells);
    rc |= ba_exact_trace_check_lengths(len, len, 4);
    return rc;
}
"""


def test_exact_cigars_symbols_are_exported(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_exact_cigars_calls_are_declared(tmp_path):
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


def test_trace_limit_names_the_pair(hip):
    """|q| * |r| <= BA_EXACT_TRACE_MAX_CELLS = 2^31 (and the int32 guard of the scores). Lengths only: nothing is allocated."""
    assert hip.EXACT_TRACE_MAX_CELLS == 1 << 31
    hip.exact_trace_check_lengths([10, 1 << 16, 1 << 20, 0], [10, 1 << 15, 1 << 11, (1 << 23) - 1])      # pairs 1 and 2 are at the limit
    with pytest.raises(RuntimeError, match=r"pair 2 .*too large for a traced matrix.*2147483648"):
        hip.exact_trace_check_lengths([10, 1 << 16, (1 << 16) + 1], [10, 1 << 15, 1 << 15])
    with pytest.raises(RuntimeError, match=r"pair 1 .*too large"):
        hip.exact_trace_check_lengths([5, 46341], [5, 46342])
    assert 46341 * 46342 > 1 << 31 >= 46340 * 46341
    hip.exact_trace_check_lengths([46340], [46341])
    with pytest.raises(RuntimeError, match=r"pair 0 .*too long"):                                        # the scores' guard comes first
        hip.exact_trace_check_lengths([1 << 23], [1])
    L = hip.lib()
    assert L.ba_exact_trace_check_lengths(None, None, 3) != 0 and "null" in hip.last_error()
    assert L.ba_exact_trace_check_lengths(None, None, 0) == 0


def test_null_arguments_are_refused(hip):
    L = hip.lib()
    rec, off = np.zeros(2, hip.EXACT_DTYPE), np.zeros(3, np.uint64)
    for f in (L.ba_batch_exact_cigars, L.ba_sized_batch_exact_cigars, L.ba_multibatch_exact_cigars):
        assert f(None, 0, -1, None, 0, rec.ctypes.data, off.ctypes.data, None, 0) != 0
        assert "null batch" in hip.last_error()
        assert f(None, 0, -1, None, 0, None, None, None, 0) != 0 and hip.last_error()
    ms, cells = ctypes.c_float(), ctypes.c_uint64()
    assert L.ba_batch_exact_cigars_ms(None, ctypes.byref(ms), ctypes.byref(cells)) != 0 and "null batch" in hip.last_error()


def test_python_surface(hip):
    assert callable(hip.BatchAligner.exact_cigars) and callable(hip.BatchAligner.exact_cigars_ms)
    assert callable(hip.SizedBatchAligner.exact_cigars) and callable(hip.MultiBatchAligner.exact_cigars)
    eb = object.__new__(hip.ExtendBatchAligner)          # (no device: the class alone)
    assert not hasattr(eb, "exact_cigars")
