"""Instruction budget of k_multi's loop of steps, read from the assembly the way tests/test_step_loop_isa.py reads it (the class-8 NUC unit compiled
for gfx950 with the Makefile's flags, the loop found by tools/dev/isa_loop.py). No GPU needed.

The headline instantiation, k_multi<8, NUC, trace, xdrop, 0, 128, 8, 4>: its hot path holds no scratch operation, no call, and at most
HOT_PATH_VALU_MAX vector instructions. The hot path is the loop minus the basic blocks that run only in the iteration that ends it; the loop has
no such block (the commit is one straight-line form for every iteration), so the whole loop is counted, which can only overstate the hot path.

The score-only instantiation, k_multi<8, NUC, -, xdrop, 0, 128, 8, 4>, must not grow from its count at commit b1f09c1, read with the same tool from the
same unit of that tree. Where the counts come from: profiles/r08_isa_budget.md.
"""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
TRACED = "_ZN2ba7k_multiILi8ELi1ELb1ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"
SCORE_ONLY = "_ZN2ba7k_multiILi8ELi1ELb0ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"
HOT_PATH_VALU_MAX = 966   # (983 at commit b1f09c1; 968 is the bound set for a loop whose trace words keep their cell order)
SCORE_ONLY_VALU_AT_B1F09C1 = 688

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")


def isa_loop_tool():
    spec = importlib.util.spec_from_file_location("isa_loop", os.path.join(ROOT, "tools", "dev", "isa_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    asm = tmp_path_factory.mktemp("isa") / "k.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-DBA_KIND=1", "-DBA_PMAX=8",
                        "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "ba_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return asm.read_text()


def loop_of_steps(text, symbol):
    assert symbol + ":" in text, symbol
    loop, hdr, _ = isa_loop_tool().loop_of(text, symbol + ":")
    valu = [i for i in loop if i.startswith("v_")]
    assert sum(i.startswith("v_max_i32_dpp") for i in loop) >= 32, "the eight columns' lane scans are not in this loop"
    return loop, valu, hdr


def test_headline_hot_path_budget(assembly):
    loop, valu, hdr = loop_of_steps(assembly, TRACED)
    print("traced loop of steps at", hdr, ":", len(loop), "instructions,", len(valu), "vector,", sum(i.startswith("v_cndmask") for i in loop), "v_cndmask")
    assert not [i for i in loop if i.startswith("scratch_")]
    assert not any("s_swappc" in i or "s_call" in i for i in loop), "a call inside the loop of steps"
    assert len(valu) <= HOT_PATH_VALU_MAX, len(valu)


def test_score_only_loop_does_not_grow(assembly):
    loop, valu, hdr = loop_of_steps(assembly, SCORE_ONLY)
    print("score-only loop of steps at", hdr, ":", len(loop), "instructions,", len(valu), "vector")
    assert len(valu) <= SCORE_ONLY_VALU_AT_B1F09C1, len(valu)
