"""k_multi's loop of steps reads what changes only with a slot's pair from LDS: the two sequence images and their lengths, where the trace
slot's words and records start, and the record count at which the slot has no room for another step (one compare in place of the record and
trace-word compares). The top of the trace stack is derived from the record count; a rectangle's record is one four-word store.

Small batches through the development library's switches, at the shapes where that code can go wrong: slots that leave the loop in most
visits (with one to four slots leaving at once, dead slots, empty and one-base pairs), trace slots so small that the capacity compare sends
slots out and pairs are run again, the 256- and 512-cell slot forms, and the special modes whose zero mask sits behind the trace words.
Every pair is compared with the oracle on score, both end positions, cells and every CIGAR run.
"""
import numpy as np
import pytest

from block_aligner_amd import synth
from tests.test_gpu_parity import NUC
from tests.test_gpu_pipelines import MODES, flat_oracle_runs, mode_bits

pytestmark = pytest.mark.gpu

GAPS = (-5, -1)


@pytest.fixture
def force_multi(devlib, monkeypatch):
    monkeypatch.setenv("BA_FORCE_MULTI", "1")


_pair_cells = {}   # (pairs, size, x_drop, mode) -> the oracle's cell count of every pair (its batch call returns their sum only); computed once


def oracle_cells(oracle, pairs, size, x_drop, mode):
    key = (id(pairs), size, x_drop, tuple(mode))
    if key not in _pair_cells:
        _pair_cells[key] = (pairs, np.array([oracle.align(NUC, pairs.query(p), pairs.reference(p), GAPS, size, x_drop, tuple(mode), cigar_eq="trace" in mode)["cells"]
                                             for p in range(len(pairs))], np.int64))   # (the batch is kept: its id stays its own)
    return _pair_cells[key][1]


def every_pair_equals(H, oracle, pairs, size, x_drop, mode, kernel="k_multi", want_retried=False):
    b = H.BatchAligner(NUC, GAPS, size, x_drop, mode_bits(H, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    assert b.info()["kernel"] == kernel, b.info()
    b.run()
    if want_retried:
        assert b.retried() > 0
    res = b.results()
    ref = oracle.batch_align(NUC, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, GAPS, size, x_drop, mode, cigar_eq="trace" in mode, threads=16)
    what = (size, mode, len(pairs))
    assert not res["status"].any(), (what, np.nonzero(res["status"])[0][:10])
    for got, want in (("score", ref["scores"]), ("query_idx", ref["query_idx"]), ("reference_idx", ref["reference_idx"]), ("cells", oracle_cells(oracle, pairs, size, x_drop, mode))):
        bad = np.nonzero(res[got].astype(np.int64) != np.asarray(want).astype(np.int64))[0]
        assert bad.size == 0, (what, got, bad[:10], res[got][bad[:5]], np.asarray(want)[bad[:5]])
    if "trace" in mode:
        assert np.array_equal(res["cigar_len"], ref["cig_len"]), what
        runs, off = b.cigars(res["cigar_len"])
        assert np.array_equal(runs[: int(off[len(pairs)])], flat_oracle_runs(ref, len(pairs))), what
    b.close()


def indel_pairs(n, length, seed, extra=()):
    """Related DNA pairs; every third one carries an indel of 40..200 bases, which takes its slot out of the loop of steps (a grow, solo mode, the
    way back into a slot)."""
    plain = synth.make_pairs(n, length, (20, 120), 40, synth.DNA, seed=seed)
    gapped = synth.make_pairs(n, length, (20, 120), 40, synth.DNA, seed=seed + 1, indels=1, indel_len=(40, 200))
    lists = list(extra)
    for p in range(n - len(lists)):
        src = gapped if p % 3 == 0 else plain
        lists.append((src.query(p), src.reference(p)))
    return synth.PairSet.from_lists(lists)


EDGE_PAIRS = ((b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"G", b"ACGTACGT"))


@pytest.fixture(scope="module")
def transition_pairs():
    return indel_pairs(600, (1500, 3000), 8101, EDGE_PAIRS)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", [(128, 512), (128, 1024)])
def test_transitions(hip, oracle, force_multi, transition_pairs, mode, size):
    """600 pairs of 1500..3000 bp, empty and one-base pairs among them: slots leave the loop in most visits."""
    every_pair_equals(hip, oracle, transition_pairs, size, 80, mode)


@pytest.mark.parametrize("mode", MODES)
def test_three_pairs_leave_a_wave_with_a_dead_slot(hip, oracle, force_multi, mode):
    every_pair_equals(hip, oracle, indel_pairs(3, (1500, 3000), 8111), (128, 512), 80, mode)


@pytest.mark.parametrize("mode", [("trace",), ("trace", "x_drop")])
@pytest.mark.parametrize("size", [(128, 512), (128, 1024)])
def test_capacity_compare_sends_slots_out(hip, oracle, force_multi, transition_pairs, monkeypatch, mode, size):
    """Trace slots at the smallest margin: a slot reaches its record limit inside the loop of steps, the pair reports the overflow and is run again."""
    monkeypatch.setenv("BA_ADAPTIVE_TRACE", "1")
    monkeypatch.setenv("BA_TRACE_MARGIN_PCT", "1")
    every_pair_equals(hip, oracle, transition_pairs, size, 80, mode, want_retried=True)


@pytest.mark.parametrize("mode", [("trace",), ("trace", "x_drop")])
@pytest.mark.parametrize("size", [(256, 1024), (512, 2048)])
def test_slot_widths(hip, oracle, force_multi, mode, size):
    """Two slots of 256 cells, one slot of 512 cells per wave: 300 pairs of 4..6 kbp."""
    every_pair_equals(hip, oracle, indel_pairs(300, (4000, 6000), 8121 + size[0]), size, 100, mode)


@pytest.mark.parametrize("mode", [("trace", "x_drop", "local_start"), ("trace", "local_start"), ("trace", "free_query_start_gaps"), ("trace", "x_drop", "free_query_start_gaps")])
def test_special_modes(hip, oracle, force_multi, mode):
    """LOCAL_START (a zero mask behind every rectangle's trace words) and FREE_QUERY_START_GAPS in the slots: related cores behind unrelated heads,
    queries inside longer references, ordinary pairs."""
    rng = np.random.default_rng(8131)
    base = indel_pairs(300, (1500, 3000), 8132)
    lists = []
    for p in range(len(base)):
        q, r = np.frombuffer(base.query(p), np.uint8), np.frombuffer(base.reference(p), np.uint8)
        if p % 3 == 1:
            q = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 300)), synth.DNA), q]); r = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 300)), synth.DNA), r])
        elif p % 3 == 2:
            r = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 500)), synth.DNA), r])
        lists.append((q.astype(np.uint8).tobytes(), r.astype(np.uint8).tobytes()))
    every_pair_equals(hip, oracle, synth.PairSet.from_lists(lists), (128, 512), 80, mode)
