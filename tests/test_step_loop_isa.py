"""The headline instantiation -- ba::k_multi<8, NUC, trace, xdrop, 0, 128, 8, 4>, the one bench.py's flagship launch runs -- is compiled for gfx950
with the Makefile's flags and its loop of steps is read back from the assembly: the loop around the kernel's largest basic block (the eight
unrolled columns of multi_rect), as tools/dev/isa_loop.py finds it. No GPU needed.

The loop must hold no scratch operation: a value the register allocator keeps in scratch memory is reloaded in every step behind every
outstanding memory operation (the slot's LDS addresses were, until round 7: they are derived from the lane number in every step now).
"""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
HEADLINE = "_ZN2ba7k_multiILi8ELi1ELb1ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"


def isa_loop_tool():
    """tools/dev/isa_loop.py, the tool a developer reads the same loop with"""
    spec = importlib.util.spec_from_file_location("isa_loop", os.path.join(ROOT, "tools", "dev", "isa_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
def test_headline_loop_of_steps_has_no_scratch_operation(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    asm = tmp_path / "k.s"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-sched-strategy=max-ilp", "-DBA_KIND=1", "-DBA_PMAX=8",
                        "-S", "--cuda-device-only", "-o", str(asm), os.path.join(csrc, "ba_kernels.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    text = asm.read_text()
    assert HEADLINE + ":" in text, "the headline instantiation is not in the class-8 NUC object"
    loop, hdr, _ = isa_loop_tool().loop_of(text, HEADLINE + ":")
    valu = [i for i in loop if i.startswith("v_")]
    print("loop of steps at", hdr, ":", len(loop), "instructions,", len(valu), "vector")
    assert len(valu) > 500, "this is not the loop of steps"
    assert sum(i.startswith("v_max_i32_dpp") for i in loop) >= 32, "the eight columns' lane scans are not in this loop"
    scratch = [i for i in loop if i.startswith("scratch_")]
    assert not scratch, scratch
    assert not any("s_swappc" in i for i in loop), "a call inside the loop of steps"
