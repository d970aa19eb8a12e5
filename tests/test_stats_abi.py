"""Per-alignment statistics without a GPU: the C calls are exported and declared, struct BaAlignStats has the layout the Python binding
reads, null arguments are refused with a message, and the statistics kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_batch_stats", "ba_sized_batch_stats", "ba_multibatch_stats", "ba_extend_batch_stats")


def test_stats_symbols_are_exported(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert not [n for n in CALLS + ("ba_batch_stats_ms",) if not hasattr(lib, n)]


def _caller(hip):
    checks = "\n".join(f"    _Static_assert(offsetof(struct BaAlignStats, {f}) == {getattr(hip.AlignStatsC, f).offset}, \"{f}\");"
                       for f, _ in hip.AlignStatsC._fields_)
    return f"""
#include <stddef.h>
#include "block_aligner_hip.h"
_Static_assert(sizeof(struct BaAlignStats) == 48, "BaAlignStats is 48 bytes");
int use(BaBatch* b, BaSizedBatch* s, BaMultiBatch* m, BaExtendBatch* e, struct BaAlignStats* out) {{
{checks}
    float ms = 0.0f;
    int rc = ba_batch_stats(b, out) | ba_sized_batch_stats(s, out) | ba_multibatch_stats(m, out) | ba_extend_batch_stats(e, out);
    rc |= ba_batch_stats_ms(b, &ms);
    return rc + (out->path_score < 0) + (int)out->q_start;
}}
"""


def test_stats_calls_are_declared_with_the_binding_layout(hip, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    assert ctypes.sizeof(hip.AlignStatsC) == 48 and hip.STATS_DTYPE.itemsize == 48
    src = tmp_path / "caller.c"
    src.write_text(_caller(hip))
    # (_Static_assert is C11; gcc accepts it in C99 mode without -pedantic)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("call", CALLS)
def test_null_arguments_are_refused(hip, call):
    f = getattr(hip.lib(), call)
    assert f(None, None) != 0
    assert "null batch" in hip.last_error()
    out = (hip.AlignStatsC * 4)()
    assert f(None, ctypes.byref(out)) != 0 and "null batch" in hip.last_error()
    assert hip.lib().ba_batch_stats_ms(None, None) != 0 and "null argument" in hip.last_error()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_stats_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_stats.hip"), "-o", str(tmp_path / "ba_stats.o")], capture_output=True, text=True)
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
    for k in ("k_stats", "k_stats_extend"):
        hits = [v for f, v in scratch.items() if re.search(rf"\d{k}N", f)]
        assert hits == [0], (k, scratch)
