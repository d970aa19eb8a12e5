"""k_multi's loop of steps issues every vector-memory instruction in every step, by every slot, in one order (round 10): a slot's first fetch is
issued before the loop, a slot that may not take its next step ends the loop before that step, a dead slot reads and writes addresses of its own,
the record is stored by every lane of its slot, a step's trace words are stored at the top of the next step (the last step's behind the loop), and
batches whose sequence pool does not fit in 32 bits run a kernel of their own.

Small batches through the development library's switches (BA_FORCE_MULTI), at the shapes where each of these can go wrong. Every pair is compared
with the oracle on score, both end positions, cells and every CIGAR run. Modelled on tests/test_gpu_step_peel.py; the oracle's results of a batch
are computed once and shared by the tests that run it again under another switch.

A wave of 128-cell slots enters the loop of steps only with all four slots live, and the host gives a small batch one wave per pair: left to itself
a batch of 600 pairs runs mostly solo, to the end. So every batch here runs on a few workgroups (BA_GRID) that take their pairs four at a time
(BA_WORK_CHUNK), in the eight-wave workgroups of the headline kernel (BA_MQ_GEOM=0): a wave works through a dozen pairs and more, its slots
leave and come back. That the loop was what ran is asserted, not assumed: under BA_COUNT_STEPS the kernels count the steps their slots take in
the loop -- k_multi and k_multi_p64 each into a counter of its own --, read here with ba_batch_prof.
"""
import ctypes as C

import numpy as np
import pytest

from block_aligner_amd import synth
from tests.test_gpu_parity import NUC
from tests.test_gpu_pipelines import MODES, flat_oracle_runs, mode_bits

pytestmark = pytest.mark.gpu

GAPS = (-5, -1)
TRACED = [("trace",), ("trace", "x_drop")]


@pytest.fixture
def force_multi(devlib, monkeypatch):
    monkeypatch.setenv("BA_FORCE_MULTI", "1")
    monkeypatch.setenv("BA_MQ_GEOM", "0")
    monkeypatch.setenv("BA_GRID", "4")          # 32 waves: 600 pairs are about nineteen to a wave
    monkeypatch.setenv("BA_WORK_CHUNK", "4")    # ... taken four at a time: a wave's four slots fill at once
    monkeypatch.setenv("BA_COUNT_STEPS", "1")


def slot_steps(H, b):
    """(steps taken in k_multi's loop of steps, in k_multi_p64's) by the batch's last run: the development counters of BA_COUNT_STEPS."""
    prof = np.zeros(128, np.uint64)
    fn = H.lib().ba_batch_prof
    fn.argtypes = [C.c_void_p, C.c_void_p]
    assert fn(b._h, prof.ctypes.data) == 0
    return int(prof[48]), int(prof[49])


_refs = {}   # (pairs, size, x_drop, mode) -> (the batch, the oracle's batch results, its cell count of every pair); computed once, never changed


def oracle_results(oracle, pairs, size, x_drop, mode):
    key = (id(pairs), size, x_drop, tuple(mode))
    if key not in _refs:
        ref = oracle.batch_align(NUC, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, GAPS, size, x_drop, mode, cigar_eq="trace" in mode, threads=16)
        cells = np.array([oracle.align(NUC, pairs.query(p), pairs.reference(p), GAPS, size, x_drop, tuple(mode), cigar_eq="trace" in mode)["cells"]
                          for p in range(len(pairs))], np.int64)   # (the batch call returns their sum only)
        _refs[key] = (pairs, ref, cells)   # (the batch is kept: its id stays its own)
    return _refs[key][1], _refs[key][2]


def every_pair_equals(H, oracle, pairs, size, x_drop, mode, want_retried=False, min_steps=None, p64=False):
    """min_steps: how many steps the slots must have taken in the loop of steps, at the least. None: a tenth of the steps the batch would take at the
    minimum block size, (|q| + |r|) / 8 per pair -- a slot steps only at that size; two pairs of three are related without an indel and stay there
    for most of their length, and a tenth leaves room for the stretches at larger blocks and for pairs that are run again."""
    b = H.BatchAligner(NUC, GAPS, size, x_drop, mode_bits(H, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    assert b.info()["kernel"] == "k_multi" and b.info()["geometry"] == 0, b.info()
    b.run()
    if want_retried:
        assert b.retried() > 0
    what = (size, mode, len(pairs))
    steps32, steps64 = slot_steps(H, b)
    if min_steps is None:
        min_steps = int((np.asarray(pairs.q_len, np.int64) + np.asarray(pairs.r_len, np.int64)).sum()) // 8 // 10
    print("slot steps", what, "k_multi", steps32, "k_multi_p64", steps64, "at least", min_steps)
    # (the large-pool form is a kernel of its own for traced batches: which of the two ran is which counter moved)
    took, other = (steps64, steps32) if p64 else (steps32, steps64)
    assert other == 0 and took >= min_steps, (what, steps32, steps64, min_steps)
    res = b.results()
    ref, cells = oracle_results(oracle, pairs, size, x_drop, mode)
    assert not res["status"].any(), (what, np.nonzero(res["status"])[0][:10])
    for got, want in (("score", ref["scores"]), ("query_idx", ref["query_idx"]), ("reference_idx", ref["reference_idx"]), ("cells", cells)):
        bad = np.nonzero(res[got].astype(np.int64) != np.asarray(want).astype(np.int64))[0]
        assert bad.size == 0, (what, got, bad[:10], res[got][bad[:5]], np.asarray(want)[bad[:5]])
    if "trace" in mode:
        assert np.array_equal(res["cigar_len"], ref["cig_len"]), what
        runs, off = b.cigars(res["cigar_len"])
        assert np.array_equal(runs[: int(off[len(pairs)])], flat_oracle_runs(ref, len(pairs))), what
    b.close()


def indel_pairs(n, length, seed, extra=()):
    """Related DNA pairs; every third one carries an indel of 40..200 bases, which takes its slot out of the loop of steps (a grow, solo mode, the
    way back into a slot: a first fetch before the loop)."""
    plain = synth.make_pairs(n, length, (20, 120), 40, synth.DNA, seed=seed)
    gapped = synth.make_pairs(n, length, (20, 120), 40, synth.DNA, seed=seed + 1, indels=1, indel_len=(40, 200))
    lists = list(extra)
    for p in range(n - len(lists)):
        src = gapped if p % 3 == 0 else plain
        lists.append((src.query(p), src.reference(p)))
    return synth.PairSet.from_lists(lists)


# empty and one-base pairs, and a query of 4 bases on a reference of 8
EDGE_PAIRS = ((b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"ACGT", b"ACGTACGT"))
SIZES = [(128, 512), (128, 1024)]


@pytest.fixture(scope="module")
def reentry_pairs():
    return indel_pairs(600, (1500, 3000), 10101, EDGE_PAIRS)


_few = {}


def few_pairs(n):
    if n not in _few:
        _few[n] = indel_pairs(n, (1500, 3000), 10110 + n)
    return _few[n]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES)
def test_fetch_before_the_loop(hip, oracle, force_multi, reentry_pairs, mode, size):
    """600 pairs of 1500..3000 bp: slots leave the loop and come back in most visits, each time with a first fetch issued before the loop. The
    two modes without X-drop are also the ones where the matrix edge makes a slot ineligible for its next step: the loop ends before that step."""
    every_pair_equals(hip, oracle, reentry_pairs, size, 80, mode)


@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("size", SIZES)
def test_capacity_limit_ends_the_loop_before_the_step(hip, oracle, force_multi, reentry_pairs, monkeypatch, mode, size):
    """Trace slots at the smallest margin: a slot has no room for its next step's record and trace words, the loop ends before that step, the pair
    reports the overflow and is run again."""
    monkeypatch.setenv("BA_ADAPTIVE_TRACE", "1")
    monkeypatch.setenv("BA_TRACE_MARGIN_PCT", "1")
    # (a slot of this margin has room for its pair's first block and some twenty steps of 128 words: a step per pair is the least they take together)
    every_pair_equals(hip, oracle, reentry_pairs, size, 80, mode, want_retried=True, min_steps=len(reentry_pairs))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_dead_slots(hip, oracle, force_multi, monkeypatch, mode, n):
    """Fewer pairs than a wave has slots, and one pair more than that. A wave of 128-cell slots does not step with a dead slot -- it runs the few
    it has solo --, so 1 and 3 pairs check that way out and only the batch of 5 steps: its first wave takes four (no pair is held back for the
    batch's ragged end: BA_MQ_DRAIN=0). The waves that do step with a dead slot are the wide ones, below."""
    monkeypatch.setenv("BA_MQ_DRAIN", "0")
    every_pair_equals(hip, oracle, few_pairs(n), (128, 512), 80, mode, min_steps=1 if n == 5 else 0)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [1, 3])
def test_dead_wide_slots(hip, oracle, force_multi, mode, n):
    """Two slots of 256 cells per wave go on stepping with one of them empty: one pair beside a slot that never held one, three pairs of which the last
    steps beside a slot whose pair is done. The dead slot reads at the pool's start and stores into its own buffers."""
    every_pair_equals(hip, oracle, few_pairs(n), (256, 1024), 80, mode, min_steps=1)


_wide = {}


@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("size", [(256, 1024), (512, 2048)])
def test_wide_slots(hip, oracle, force_multi, mode, size):
    """Two slots of 256 cells, one slot of 512 cells per wave (these go on stepping with an empty slot at the batch's end): 300 pairs of 4..6 kbp."""
    if size not in _wide:
        _wide[size] = indel_pairs(300, (4000, 6000), 10121 + size[0])
    every_pair_equals(hip, oracle, _wide[size], size, 100, mode)


@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("size", SIZES)
def test_large_pool_form(hip, oracle, force_multi, reentry_pairs, monkeypatch, mode, size):
    """BA_POOL64: the batch runs k_multi_p64, whose prefetch adds 64-bit offsets to the pool's base."""
    monkeypatch.setenv("BA_POOL64", "1")
    every_pair_equals(hip, oracle, reentry_pairs, size, 80, mode, p64=True)


@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("n", [1, 3, 5])
def test_large_pool_form_with_dead_slots(hip, oracle, force_multi, monkeypatch, mode, n):
    monkeypatch.setenv("BA_POOL64", "1")
    monkeypatch.setenv("BA_MQ_DRAIN", "0")
    every_pair_equals(hip, oracle, few_pairs(n), (128, 512), 80, mode, min_steps=1 if n == 5 else 0, p64=True)


@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("n", [1, 3])
def test_large_pool_form_with_dead_wide_slots(hip, oracle, force_multi, monkeypatch, mode, n):
    monkeypatch.setenv("BA_POOL64", "1")
    every_pair_equals(hip, oracle, few_pairs(n), (256, 1024), 80, mode, min_steps=1, p64=True)


def test_local_start_in_the_slots(hip, oracle, force_multi):
    """LOCAL_START with traceback and X-drop: a rectangle's zero mask is stored behind its trace words, one more store of every step. Related cores
    behind unrelated heads, queries inside longer references, ordinary pairs."""
    rng = np.random.default_rng(10131)
    base = indel_pairs(300, (1500, 3000), 10132)
    lists = []
    for p in range(len(base)):
        q, r = np.frombuffer(base.query(p), np.uint8), np.frombuffer(base.reference(p), np.uint8)
        if p % 3 == 1:
            q = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 300)), synth.DNA), q]); r = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 300)), synth.DNA), r])
        elif p % 3 == 2:
            r = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 500)), synth.DNA), r])
        lists.append((q.astype(np.uint8).tobytes(), r.astype(np.uint8).tobytes()))
    every_pair_equals(hip, oracle, synth.PairSet.from_lists(lists), (128, 512), 80, ("trace", "x_drop", "local_start"))
