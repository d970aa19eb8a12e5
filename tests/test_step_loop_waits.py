"""The waits on the memory counter in k_multi's loop of steps (round 10), read from the assembly the way tests/test_step_loop_budget.py reads it (the
class-8 NUC unit compiled for gfx950 with the Makefile's flags, the loop found by tools/dev/isa_loop.py). No GPU needed.

Every vector-memory instruction of the loop is issued in every step, by every slot, in one order: the previous step's trace words, the four
prefetch loads of the step after this one, the step's record. The compiler can then count them, and the only waits that name vmcnt are those in
front of the prefetched bytes' first use -- a whole step after their loads were issued --, which leave the step's stores outstanding. Read in four instantiations: the headline kernel, the score-only one, the traced one without X-drop and a traced one with 256-cell slots.

Where this stands (figures of the tree that added this file):
  traced loops (headline, without X-drop, 256-cell slots): one wait, s_waitcnt vmcnt(3), at index 28 / 5 / 29 of 1116 / 1131 / 1164 instructions,
      ahead of the loads at 132.. / 131.. / 128..; three stores a step; no exec-masked block at all.
  score-only loop: a step stores nothing, so behind its four loads nothing else would be outstanding and the wait for the last of them would read
      vmcnt(0). Its loads go out as two pairs, each right behind the wait for its own registers' bytes of the step before: s_waitcnt vmcnt(2) at
      index 33, loads at 61 and 63, s_waitcnt vmcnt(2) at 100, loads at 109 and 110, of 860 instructions. Either wait leaves the other pair in flight;
      the second one stands behind this step's first pair and does not wait for it (test_no_wait_is_for_a_load_of_its_own_step).
"""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SYMBOL = "_ZN2ba7k_multiILi8ELi1ELb%dELb%dELi0ELi%dELi8ELi4EEEvNS_11BatchParamsE"
HEADLINE = SYMBOL % (1, 1, 128)
SCORE_ONLY = SYMBOL % (0, 1, 128)
TRACED_NO_XDROP = SYMBOL % (1, 0, 128)
WIDE = SYMBOL % (1, 1, 256)
# the large-pool form of the headline kernel, a symbol of its own: its prefetch adds 64-bit offsets per lane to the pool's base
LARGE_POOL = "_ZN2ba11k_multi_p64ILi8ELi1ELb1ELi0ELi128ELi8ELi4EEEvNS_11BatchParamsE"
TRACED = [HEADLINE, TRACED_NO_XDROP, WIDE, LARGE_POOL]
ALL = [HEADLINE, SCORE_ONLY, TRACED_NO_XDROP, WIDE, LARGE_POOL]
STORES_PER_TRACED_STEP = 3   # the record and the two halves of a lane's trace words

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


_loops = {}


def loop_of_steps(text, symbol):
    """-> (the loop's instructions, {label: index of the first instruction behind it}) of the loop of steps of `symbol`"""
    if symbol not in _loops:
        assert symbol + ":" in text, symbol
        loop, hdr, _ = isa_loop_tool().loop_of(text, symbol + ":")
        assert sum(i.startswith("v_max_i32_dpp") for i in loop) >= 32, "the eight columns' lane scans are not in this loop"
        # the same lines again, with the labels between them
        lines = text.split("\n")
        k = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
        k = next(i for i in range(k, len(lines)) if lines[i].startswith(".L%s:" % hdr))
        labels, n = {}, 0
        while n < len(loop):
            t = lines[k].strip()
            m = re.match(r"^(\.LBB\d+_\d+):", lines[k])
            if m:
                labels[m.group(1)] = n
            elif t and not t.startswith((";", ".")):
                assert t == loop[n], (t, loop[n])
                n += 1
            k += 1
        _loops[symbol] = (loop, labels)
    return _loops[symbol]


def is_vmem(i):
    return i.startswith(("global_", "flat_", "buffer_", "scratch_"))


def vmcnt_waits(loop):
    """[(index, N)] of every s_waitcnt of the loop that names vmcnt"""
    out = []
    for k, i in enumerate(loop):
        m = re.match(r"s_waitcnt\b.*\bvmcnt\((\d+)\)", i)
        if m:
            out.append((k, int(m.group(1))))
    return out


def report(symbol, loop):
    loads = [k for k, i in enumerate(loop) if i.startswith(("global_load", "flat_load"))]
    stores = [k for k, i in enumerate(loop) if i.startswith(("global_store", "flat_store"))]
    print(symbol[8:40], ":", len(loop), "instructions; loads at", loads, "stores at", stores, "vmcnt waits", vmcnt_waits(loop),
          "s_cbranch_execz at", [k for k, i in enumerate(loop) if i.startswith("s_cbranch_execz")])
    return loads, stores


@pytest.mark.parametrize("symbol", ALL)
def test_loads_are_the_prefetch_and_nothing_waits_behind_them(assembly, symbol):
    loop, _ = loop_of_steps(assembly, symbol)
    loads, stores = report(symbol, loop)
    # the loop's loads are exactly the four prefetch loads (eight bytes each: a lane's cells of the vector axis, the step's columns; both directions)
    assert len(loads) == 4 and all(loop[k].startswith("global_load_dwordx2") for k in loads), [loop[k] for k in loads]
    if symbol not in (SCORE_ONLY, LARGE_POOL):   # (traced: the pool's base in scalar registers, a 32-bit offset per lane -- the 32-bit loop, not the large-pool form's)
        assert all(re.match(r"global_load_dwordx2 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]", loop[k]) for k in loads), [loop[k] for k in loads]
    # no wait on the memory counter between them and the loop's back edge: they are in flight until the next step
    # (score only: behind the LAST load. Its second wait stands behind the first pair of loads, which is short of "no wait follows the loads"
    # read strictly; that this wait does not wait for that pair is what test_no_wait_is_for_a_load_of_its_own_step asserts, for every wait and load)
    behind = [(k, n) for k, n in vmcnt_waits(loop) if k > loads[-1]]
    assert not behind, behind
    if symbol != SCORE_ONLY:   # (the traced loops issue the four together: nothing waits behind the first of them either)
        assert not [(k, n) for k, n in vmcnt_waits(loop) if k > loads[0]]
    assert not [i for i in loop if i.startswith("flat_")]


@pytest.mark.parametrize("symbol", ALL)
def test_no_wait_is_for_a_load_of_its_own_step(assembly, symbol):
    """The counter is in order: s_waitcnt vmcnt(N) at k lets the last N vector-memory instructions stay outstanding, so it waits for a load issued at
    i < k of the same step exactly when N or more such instructions were issued between the two. No wait of the loop may wait for a load of its
    own step: a load is waited for in the step after the one that issued it."""
    loop, _ = loop_of_steps(assembly, symbol)
    loads, _ = report(symbol, loop)
    for k, n in vmcnt_waits(loop):
        for i in loads:
            if i < k:
                issued_since = sum(is_vmem(loop[j]) for j in range(i + 1, k))
                assert issued_since < n, (k, loop[k], i, loop[i], issued_since)   # (the load is among the N that may stay outstanding)


@pytest.mark.parametrize("symbol", ALL)
def test_every_wait_leaves_the_steps_stores_outstanding(assembly, symbol):
    loop, _ = loop_of_steps(assembly, symbol)
    loads, stores = report(symbol, loop)
    if symbol == SCORE_ONLY:
        assert not stores, [loop[k] for k in stores]
    else:
        assert len(stores) == STORES_PER_TRACED_STEP, [loop[k] for k in stores]
    short = [(k, n) for k, n in vmcnt_waits(loop) if n < len(stores)]
    assert not short, short


def test_score_only_loop_has_no_vmcnt0(assembly):
    loop, _ = loop_of_steps(assembly, SCORE_ONLY)
    report(SCORE_ONLY, loop)
    assert not [(k, n) for k, n in vmcnt_waits(loop) if n == 0], vmcnt_waits(loop)


@pytest.mark.parametrize("symbol", ALL)
def test_no_memory_instruction_in_an_exec_masked_block(assembly, symbol):
    """No vector-memory instruction lies between an s_cbranch_execz and its target: what a slot or a step may skip, the compiler cannot count."""
    loop, labels = loop_of_steps(assembly, symbol)
    for k, i in enumerate(loop):
        if not i.startswith("s_cbranch_execz"):
            continue
        target = i.split()[-1]
        end = labels.get(target, len(loop))   # (a target outside the loop: everything up to the loop's end)
        lo, hi = (k + 1, end) if end > k else (end, k)
        inside = [(j, loop[j]) for j in range(lo, hi) if is_vmem(loop[j])]
        assert not inside, (k, i, inside)


def written(i):
    """the vector registers an instruction writes: its first operand, v7 or v[4:7]"""
    m = re.match(r"\S+\s+v(\d+)\b|\S+\s+v\[(\d+):(\d+)\]", i)
    if not m or i.startswith(("global_store", "ds_write", "s_", "v_cmp", "v_nop")):
        return set()
    return {int(m.group(1))} if m.group(1) else set(range(int(m.group(2)), int(m.group(3)) + 1))


@pytest.mark.parametrize("symbol", [HEADLINE, TRACED_NO_XDROP, WIDE, LARGE_POOL])
def test_nothing_puts_the_trace_bytes_in_order_before_the_stores(assembly, symbol):
    """A step's trace words are stored at the top of the next step, so no instruction stands between the loop's header and the two stores, and the
    check of tests/test_trace_word_order.py -- no v_perm_b32 in the branch-free code in front of the stores -- reads an empty region there: it
    holds, and says nothing. This is that check across the back edge: each of the eight registers the two stores read is followed back from the
    loop's end to the instruction that wrote it (through plain moves), and that instruction is the column code's last bit-field insert into the
    word, not a v_perm_b32 that reorders its bytes."""
    loop, _ = loop_of_steps(assembly, symbol)
    pairs = [k for k in range(len(loop) - 1) if loop[k].startswith("global_store_dwordx4") and loop[k + 1].startswith("global_store_dwordx4") and "offset:16" in loop[k + 1]]
    assert len(pairs) == 1, pairs
    regs = []
    for k in (pairs[0], pairs[0] + 1):
        m = re.match(r"global_store_dwordx4 v\S+, v\[(\d+):(\d+)\]", loop[k])
        assert m, loop[k]
        regs += list(range(int(m.group(1)), int(m.group(2)) + 1))
    assert len(regs) == 8, regs
    # the instructions of one turn of the loop that run before the stores, latest first: the few at the loop's top, then the step before from its end
    before = [loop[k] for k in range(pairs[0] - 1, -1, -1)] + [loop[k] for k in range(len(loop) - 1, pairs[0] + 1, -1)]
    writers = []
    for r in regs:
        at = -1
        for hops in range(4):   # (a move or two between the column code's register and the store's)
            at = next((k for k in range(at + 1, len(before)) if r in written(before[k])), None)
            assert at is not None, (r, "is not written in the loop")
            w = before[at]
            m = re.match(r"v_mov_b32(?:_e32)? v\d+, v(\d+)$", w)
            if not m:
                break
            r = int(m.group(1))
        writers.append(w.split()[0])
    print(symbol[8:44], "the stored trace words are written by", writers)
    assert all(w.startswith("v_bfi_b32") for w in writers), writers
