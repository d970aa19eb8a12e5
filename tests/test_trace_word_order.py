"""Trace words of k_multi's slot rectangles in the order of its registers (round 9). No GPU needed.

(a) The byte map. A lane's 8 cells x 2 columns are the 8 bytes of two consecutive trace words. Until round 9 byte c held cell c (word c >> 2 held
cells 0 .. 3 or 4 .. 7: still k_small's order); k_multi now stores word p2 as its register pair holds it, cells (2 p2, 2 p2 + 1, 2 p2 + 4, 2 p2 + 5) in
bytes 0 .. 3, so cell c = (b2 b1 b0) is byte b1 * 4 + b2 * 2 + b0. The device states the map once, as slot_cell_byte<RO> in ba_driver.hpp; here it is
stated in Python and composed with the window address every lane walker uses -- byte (row >> 3) * 32 + (column >> 1) * 8 + [cell's byte] of a
window of 16 rows x 8 columns -- to give the tables tb_diag must hold:
    F[u][k] = (x >> 3) * 32 + cell_byte(x & 7)  with x = (u - k) & 15        (u = row in the window, k = steps up the diagonal)
    G[w][k] = (((w - k) & 7) >> 1) * 8                                       (w = column)
    F[u][k] + G[w][k] = the byte of cell (u - k, w - k) for every k <= min(u, w).
What the device computes with these is checked on the GPU (tests/test_gpu_trace_word_order.py).

(b) The loop of steps, read as tests/test_step_loop_budget.py reads it (same flags, same tool): the traced headline loop holds no flat load and no
scratch operation, the v_perm_b32 that put the trace bytes in cell order ahead of the step's two trace stores are gone, and the loop is within
TRACED_VALU_MAX vector instructions. The round's bound was 958 = 966 less those eight v_perm; with the sequence prefetch by 32-bit offset the loop
reads 955, and that is the bound (profiles/r09_isa_budget.md, section 1). The score-only loop must not grow (688).
"""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
TRACED = "_ZN2ba7k_multiILi8ELi1ELb1ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"
SCORE_ONLY = "_ZN2ba7k_multiILi8ELi1ELb0ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"
TRACED_VALU_MAX = 955   # (958 with the trace words in register order alone)
SCORE_ONLY_VALU_MAX = 688


# ---------------------------------------------------------------- (a)
def cell_byte(c, register_order=True):
    """byte of cell c = 0 .. 7 of a lane among the 8 bytes of a column pair (slot_cell_byte<RO> of ba_driver.hpp)"""
    if not register_order:
        return c
    b0, b1, b2 = c & 1, (c >> 1) & 1, (c >> 2) & 1
    return b1 * 4 + b2 * 2 + b0


def window_byte(row, col, register_order):
    """byte of cell (row, col) in a lane walker's window of 16 rows x 8 columns: two lanes' 32-byte groups, word (col >> 1) * 2 + p2 in each"""
    return (row >> 3) * 32 + (col >> 1) * 8 + cell_byte(row & 7, register_order)


def test_byte_map_and_diagonal_tables():
    assert [cell_byte(c) for c in range(8)] == [0, 1, 4, 5, 2, 3, 6, 7]
    assert sorted(cell_byte(c) for c in range(8)) == list(range(8))
    assert [cell_byte(c, False) for c in range(8)] == list(range(8))
    # word p2 of a column pair holds cells (2 p2, 2 p2 + 1, 2 p2 + 4, 2 p2 + 5) in bytes 0 .. 3: what multi_rect's sign gathers produce
    for p2 in range(2):
        cells = sorted(range(8), key=cell_byte)[4 * p2: 4 * p2 + 4]
        assert cells == [2 * p2, 2 * p2 + 1, 2 * p2 + 4, 2 * p2 + 5]
    # composed with the old word and byte address: the same word group, the same column pair, only the byte inside the pair's 8 moves
    for row in range(16):
        for col in range(8):
            old, new = window_byte(row, col, False), window_byte(row, col, True)
            assert old == (row >> 3) * 32 + (col >> 1) * 8 + (row & 7)
            assert new - (new & 7) == old - (old & 7) and (new & 7) == cell_byte(old & 7)
    # tb_diag's tables
    for order in (False, True):
        F = [[(((u - k) & 15) >> 3) * 32 + cell_byte(((u - k) & 15) & 7, order) for k in range(8)] for u in range(16)]
        G = [[(((w - k) & 7) >> 1) * 8 for k in range(8)] for w in range(8)]
        assert all(0 <= v < 64 for t in F + G for v in t)
        for u in range(16):
            for w in range(8):
                for k in range(min(u, w, 7) + 1):
                    assert F[u][k] + G[w][k] == window_byte(u - k, w - k, order), (order, u, w, k)
    # the words' bytes as the whole-wave walk and the one-lane walk address them: word (v >> 3) * 8 + (w >> 1) * 2 + (byte >> 2), shift (byte & 3) * 8 + (w & 1) * 4
    for v in range(128):
        for w in range(8):
            b = cell_byte(v & 7)
            word, shift = (v >> 3) * 8 + (w >> 1) * 2 + (b >> 2), (b & 3) * 8 + (w & 1) * 4
            assert word * 32 + shift == ((v >> 3) * 32 + (w >> 1) * 8 + b) * 8 + (w & 1) * 4


def test_the_device_states_the_map_once():
    """One constexpr function in ba_driver.hpp, used by every reader of a slot rectangle's words and named where multi_rect writes them."""
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    with open(os.path.join(csrc, "ba_driver.hpp")) as f:
        drv = f.read()
    assert len(re.findall(r"constexpr uint32_t slot_cell_byte\(uint32_t c\)", drv)) == 1
    assert "((c & 2u) << 1) | ((c & 4u) >> 1) | (c & 1u)" in drv
    assert drv.count("slot_cell_byte<RO>(") >= 6   # traceback, walk_wave (two places), tb_step, tb_diag's F table, tb_step_fast
    with open(os.path.join(csrc, "ba_multi.hpp")) as f:
        assert "slot_cell_byte<true>" in f.read()


# ---------------------------------------------------------------- (b)
def isa_loop_tool():
    spec = importlib.util.spec_from_file_location("isa_loop", os.path.join(ROOT, "tools", "dev", "isa_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
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


def test_traced_loop_of_steps(assembly):
    loop, valu, hdr = loop_of_steps(assembly, TRACED)
    loads = [i for i in loop if i.startswith(("flat_load", "global_load"))]
    print("traced loop of steps at", hdr, ":", len(loop), "instructions,", len(valu), "vector,", sum(i.startswith("v_perm_b32") for i in loop), "v_perm_b32; loads:", loads)
    assert not [i for i in loop if i.startswith("flat_")], "a flat memory operation in the loop of steps"
    assert not [i for i in loop if i.startswith("scratch_")]
    # the sequence prefetch: the pool's base in scalar registers, a 32-bit offset per lane
    saddr = [i for i in loads if re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", i)]
    assert len(saddr) >= 4, loads
    # the step's two trace stores (the second 16 bytes behind the first): nothing puts bytes in order in front of them
    pairs = [k for k in range(len(loop) - 1) if loop[k].startswith("global_store_dwordx4") and loop[k + 1].startswith("global_store_dwordx4") and "offset:16" in loop[k + 1]]
    assert len(pairs) == 1, pairs
    k = pairs[0]
    region = []
    while k > 0 and not loop[k - 1].startswith("s_cbranch"):
        k -= 1
        region.append(loop[k])
    assert not [i for i in region if i.startswith("v_perm_b32")], region
    assert len(valu) <= TRACED_VALU_MAX, len(valu)


def test_score_only_loop_of_steps_does_not_grow(assembly):
    loop, valu, hdr = loop_of_steps(assembly, SCORE_ONLY)
    print("score-only loop of steps at", hdr, ":", len(loop), "instructions,", len(valu), "vector")
    assert len(valu) <= SCORE_ONLY_VALU_MAX, len(valu)
