"""Alignment strings without a GPU: the C calls are exported and declared, a C99 caller compiles against the header, null batches are
refused with a message, and the text kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_batch_text", "ba_sized_batch_text", "ba_multibatch_text", "ba_extend_batch_text")


def test_text_symbols_are_exported(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert not [n for n in CALLS + ("ba_batch_text_ms",) if not hasattr(lib, n)]


CALLER = r"""
#include <stddef.h>
#include "block_aligner_hip.h"
_Static_assert(BA_TEXT_CIGAR == 0 && BA_TEXT_MD == 1 && BA_TEXT_CS == 2 && BA_TEXT_SOFT_CLIP == 256, "BA_TEXT_*");
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, BaExtendBatch* e, uint64_t* offsets, char* text, uint64_t capacity) {
    float ms = 0.0f;
    int rc = ba_batch_text(b, BA_TEXT_CIGAR | BA_TEXT_SOFT_CLIP, offsets, NULL, 0);
    rc |= ba_batch_text(b, BA_TEXT_MD, offsets, text, capacity) | ba_sized_batch_text(s, BA_TEXT_CS, offsets, text, capacity);
    rc |= ba_multibatch_text(m, BA_TEXT_MD, offsets, text, capacity) | ba_extend_batch_text(e, BA_TEXT_CIGAR, offsets, text, capacity);
    rc |= ba_batch_text_ms(b, &ms);
    return rc + (ms < 0.0f);
}
"""


def test_text_calls_are_declared(hip, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS + ("ba_batch_text_ms",):
        assert re.search(rf"\b{n}\s*\(", text), n
    assert (hip.TEXT_CIGAR, hip.TEXT_MD, hip.TEXT_CS, hip.TEXT_SOFT_CLIP) == (0, 1, 2, 256)
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("call", CALLS)
def test_null_batches_are_refused(hip, call):
    f = getattr(hip.lib(), call)
    off = (ctypes.c_uint64 * 4)()
    assert f(None, 0, None, None, 0) != 0 and "null batch" in hip.last_error()
    assert f(None, hip.TEXT_MD, ctypes.byref(off), None, 0) != 0 and "null batch" in hip.last_error()
    assert hip.lib().ba_batch_text_ms(None, None) != 0 and "null argument" in hip.last_error()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_text_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_text.hip"), "-o", str(tmp_path / "ba_text.o")], capture_output=True, text=True)
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
    for k in ("k_text_len", "k_text_write", "k_text_offsets"):
        hits = [v for f, v in scratch.items() if re.search(rf"\d{k}[NP]", f)]
        assert hits == [0], (k, scratch)
