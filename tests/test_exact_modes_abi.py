"""BA_EXACT_OWN_MODE without a GPU: the flag is declared as 256 and the binding exposes it, the new host-only call is exported and declared,
and the profile length guard refuses a pair past (|q| + |r|) * 384 < 2^30, naming it, and accepts the pair just inside."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "block_aligner_hip.h")
MAX_LEN2_PROFILE = (1 << 30) // 384 - 1
CALLER = r"""
#include "block_aligner_hip.h"
typedef char own_mode_is_256[BA_EXACT_OWN_MODE == 256 ? 1 : -1];
typedef char own_mode_is_a_flag[(BA_EXACT_OWN_MODE & (BA_EXACT_GLOBAL | BA_EXACT_EXTEND)) == 0 ? 1 : -1];
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, const uint32_t* len) {
    struct BaExact rec[4];
    int rc = ba_batch_exact(b, BA_EXACT_GLOBAL | BA_EXACT_OWN_MODE, -1, NULL, 0, rec);
    rc |= ba_sized_batch_exact(s, BA_EXACT_EXTEND | BA_EXACT_OWN_MODE, 30, NULL, 0, rec);
    rc |= ba_multibatch_exact(m, BA_EXACT_EXTEND | BA_EXACT_OWN_MODE, -1, len, 4, rec);
    return rc | ba_exact_check_lengths_profile(len, len, 4);
}
"""


def test_header_declares_the_flag_as_256():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bBA_EXACT_OWN_MODE\s*=\s*1u\s*<<\s*8\b", text)
    assert re.search(r"\bba_exact_check_lengths_profile\s*\(", text)


def test_a_c_caller_compiles_against_the_flag(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_binding_exposes_the_flag_and_the_call(hip):
    assert hip.EXACT_OWN_MODE == 256 and not hip.EXACT_OWN_MODE & (hip.EXACT_GLOBAL | hip.EXACT_EXTEND)
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), "ba_exact_check_lengths_profile"), path
    import inspect
    for cls in (hip.BatchAligner, hip.ProfileBatchAligner, hip.SizedBatchAligner, hip.MultiBatchAligner):
        for name in ("exact", "accuracy"):
            assert inspect.signature(getattr(cls, name)).parameters["own_mode"].default is False, (cls, name)


def test_profile_length_guard_names_the_pair(hip):
    """Three int8 terms per column: |q| + |r| <= 2^30 / 384 - 1. Lengths only: nothing is allocated."""
    inside = MAX_LEN2_PROFILE
    hip.exact_check_lengths_profile([10, inside - 5, 0], [10, 5, inside])
    with pytest.raises(RuntimeError, match=r"pair 2 .*profile.*too long"):
        hip.exact_check_lengths_profile([10, 5, inside - 4], [10, 5, 5])
    with pytest.raises(RuntimeError, match=r"pair 0 "):
        hip.exact_check_lengths_profile([0xffffffff], [0xffffffff])
    hip.exact_check_lengths([inside - 4], [5])            # the sequence guard is three times as wide, and unchanged
    assert hip.lib().ba_exact_check_lengths_profile(None, None, 1) != 0 and "null" in hip.last_error()


def test_kernel_hash_lists_the_new_sources():
    from tools import kernel_hash
    assert "ba_exact.hip" in kernel_hash.FILES and "ba_exact.h" in kernel_hash.FILES   # the one source of the own-mode kernels and its header
