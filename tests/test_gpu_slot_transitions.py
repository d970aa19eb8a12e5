"""k_multi's slots hold a lane's eight cells as (k, k + 4) per register inside the loop of steps and as consecutive cells everywhere else
(the arena, the per-pair driver's borders, the trace words). Every time a pair moves between a slot and solo mode its borders and its checkpoint
cross that boundary, in one direction or the other.

These batches force many such moves: DNA pairs with many SHORT insertions and deletions at 128..512, so that a pair grows for a few steps, shrinks
back to 128 cells and returns to its slot again and again; every pair is compared with the oracle (score, ends, cells, every CIGAR run).
"""
import pytest

from block_aligner_amd import synth
from tests.test_gpu_parity import NUC
from tests.test_gpu_pipelines import MODES, mode_bits, run_and_compare

pytestmark = pytest.mark.gpu


def assert_pairs_leave_their_slots(oracle, pairs, gaps, x_drop, what):
    """The batch is only worth its name if its pairs do leave the 128-cell slots. Neither the library nor `info()` counts solo episodes, so the
    oracle's own step count is used: a pair that took nothing but shift steps at 128 cells has computed exactly steps x 8 x 128 cells; every
    cell beyond that is a grow -- a step a slot cannot take, i.e. a move to solo mode and (while the pair shrinks back) into a slot again.
    Every sampled pair must have grown, and the median pair must have spent a tenth more cells than its steps at 128 cells account for."""
    ratios = []
    for p in range(0, len(pairs), max(1, len(pairs) // 48)):
        r = oracle.align(NUC, pairs.query(p), pairs.reference(p), gaps, (128, 512), x_drop, ("trace", "x_drop"), cigar_eq=True)
        ratios.append(r["cells"] / (r["steps"] * 8.0 * 128.0))
    ratios.sort()
    assert ratios[0] > 1.0 and ratios[len(ratios) // 2] >= 1.1, (what, ratios[0], ratios[len(ratios) // 2])


@pytest.mark.parametrize("mode", MODES)
def test_many_slot_to_solo_transitions(hip, oracle, mode):
    """13 k pairs of 1500..3000 bases, eight indels of 5..40 bases each besides 60..300 substitutions: 128..512 with X-drop 80."""
    pairs = synth.make_pairs(13000, (1500, 3000), (60, 300), 80, synth.DNA, seed=707, indels=8, indel_len=(5, 40))
    b = hip.BatchAligner(NUC, (-5, -1), (128, 512), 80, mode_bits(hip, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    assert b.info()["kernel"] == "k_multi"
    b.close()
    assert_pairs_leave_their_slots(oracle, pairs, (-5, -1), 80, mode)
    run_and_compare(hip, oracle, pairs, NUC, (-5, -1), (128, 512), 80, mode, True, ("dna 128..512, many short indels", mode))


@pytest.mark.parametrize("gaps", [(-4, -2), (-12, -3)])
def test_transitions_with_other_gap_costs(hip, oracle, gaps):
    """The same with steeper gap costs (the in-lane scan's constants are multiples of the extension cost), traced with X-drop."""
    mode = ("trace", "x_drop")
    pairs = synth.make_pairs(13000, (1500, 3000), (60, 300), 80, synth.DNA, seed=709, indels=6, indel_len=(5, 60))
    b = hip.BatchAligner(NUC, gaps, (128, 512), 120, mode_bits(hip, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    assert b.info()["kernel"] == "k_multi"
    b.close()
    assert_pairs_leave_their_slots(oracle, pairs, gaps, 120, gaps)
    run_and_compare(hip, oracle, pairs, NUC, gaps, (128, 512), 120, mode, True, ("dna 128..512, many short indels", gaps))
