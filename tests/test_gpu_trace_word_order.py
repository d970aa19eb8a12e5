"""GPU parity of k_multi's trace words in the order of its registers (round 9) and of the 32-bit sequence prefetch.

multi_rect stores a slot rectangle's trace words as its register pairs hold them (cells (2 p2, 2 p2 + 1, 2 p2 + 4, 2 p2 + 5) to a word), and every
walker behind k_multi reads them through slot_cell_byte<true> (ba_driver.hpp): the lanes of the traceback waves (tb_step_fast with tb_diag's
tables; tb_step for the special modes), the whole-wave walk of the helpers and of the solo driver (walk_wave), the one-lane walk of the special
modes (traceback). A reader that kept the cell order would swap cells 2, 3 with 4, 5 of every lane, so the pairs here carry 8 % edits and a few
20 .. 80-base indels: their paths leave the diagonal, cross rectangles in both orientations, and some pairs go solo and come back. k_small's
rectangles share the record bit and the walker code but keep the cell order: one of its batches runs too.

Every pair is compared with the oracle -- score, both ends, computed cells, every CIGAR run -- and a spread of pairs goes through
verify.check_cigar, which needs no oracle. An oracle result is computed once per (pairs, size, mode, CIGAR_EQ) and shared by the cases."""
import numpy as np
import pytest

from block_aligner_amd import synth, verify
from tests.test_gpu_multi import _flanked_pairs
from tests.test_gpu_parity import NUC

pytestmark = pytest.mark.gpu

GAPS, X_DROP = (-5, -1), 100
WIDTHS = [(128, 512), (256, 1024), (512, 2048)]   # slots of 16, 32 and 64 lanes (the ranges of test_multi_*, test_multi256_*, test_multi512_*)
TRACED = [("trace", "x_drop"), ("trace",)]
SPECIAL = [("trace", "local_start"), ("trace", "x_drop", "local_start"), ("trace", "free_query_start_gaps")]
_pairs, _refs, _first = {}, {}, {}


def pairs_of(what):
    if what not in _pairs:
        if what == "dna":
            _pairs[what] = synth.make_pairs(600, (1500, 3000), (120, 240), 60, synth.DNA, seed=909, indels=3, indel_len=(20, 80))
        elif what == "flanked":
            _pairs[what] = _flanked_pairs(300, 91, core=(1000, 3000), flank=400)
        else:
            _pairs[what] = synth.make_pairs(2000, (900, 1100), (40, 90), 40, synth.DNA, seed=910, indels=1, indel_len=(20, 60))
    return _pairs[what]


def reference(oracle, what, size, mode, eq):
    key = (what, size, mode, eq)
    if key not in _refs:
        p = pairs_of(what)
        _refs[key] = oracle.batch_align(NUC, p.pool, p.q_off, p.q_len, p.r_off, p.r_len, GAPS, size, X_DROP, mode, cigar_eq=eq, threads=16)
    return _refs[key]


def run_hip(H, what, size, mode, eq, kernel="k_multi"):
    p = pairs_of(what)
    bits = 0
    for m in mode:
        bits |= {"trace": H.TRACE, "x_drop": H.X_DROP, "local_start": H.LOCAL_START, "free_query_start_gaps": H.FREE_QUERY_START_GAPS}[m]
    b = H.BatchAligner(NUC, GAPS, size, X_DROP, bits | (H.CIGAR_EQ if eq else 0), p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
    assert b.info()["kernel"] == kernel, b.info()
    b.run()
    res = b.results()
    runs, off = b.cigars(res["cigar_len"])
    b.close()
    return res, np.array(runs, copy=True), np.array(off, copy=True)


def check(got, ref, what, size, mode):
    res, runs, off = got
    p = pairs_of(what)
    assert not res["status"].any(), np.nonzero(res["status"])[0][:10]
    bad = np.nonzero((res["score"] != ref["scores"]) | (res["query_idx"] != ref["query_idx"]) | (res["reference_idx"] != ref["reference_idx"]))[0]
    assert bad.size == 0, (bad[:10], res["score"][bad[:5]], ref["scores"][bad[:5]])
    assert int(res["cells"].sum()) == ref["cells"]
    assert np.array_equal(res["cigar_len"], ref["cig_len"]), np.nonzero(res["cigar_len"] != ref["cig_len"])[0][:10]
    for k in range(len(p)):
        want = ref["cig_ops"][int(ref["cig_off"][k]): int(ref["cig_off"][k]) + int(ref["cig_len"][k])]
        assert np.array_equal(runs[int(off[k]): int(off[k + 1])], want), (k, mode, size)
    for k in range(0, len(p), 23):
        verify.check_cigar(runs[int(off[k]): int(off[k + 1])], p.query(k), p.reference(k), NUC, GAPS, int(res["score"][k]), int(res["query_idx"][k]),
                           int(res["reference_idx"][k]), mode, what=("pair", k, mode, size))


@pytest.fixture
def multi(devlib, monkeypatch):
    monkeypatch.setenv("BA_FORCE_MULTI", "1")
    return devlib


@pytest.fixture
def ring(multi, monkeypatch):
    """the hand-off ring and traceback waves on a small batch, as test_multi_config3_shape_with_traceback_waves sets them up"""
    monkeypatch.setenv("BA_FORCE_TB", "1")
    monkeypatch.setenv("BA_WGS_PER_CU", "1")
    return multi


@pytest.mark.parametrize("eq", [True, False])
@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("size", WIDTHS)
def test_slots_with_traceback_waves(ring, oracle, size, mode, eq):
    """The lanes' walks (tb_step_fast, tb_diag's F table), the emptied fill waves' whole-wave walks and slot donation at the end of the batch."""
    got = run_hip(ring, "dna", size, mode, eq)
    check(got, reference(oracle, "dna", size, mode, eq), "dna", size, mode)
    _first.setdefault((size, mode, eq), got)


@pytest.mark.parametrize("eq", [True, False])
@pytest.mark.parametrize("mode", TRACED)
@pytest.mark.parametrize("size", WIDTHS)
def test_slots_walked_behind_the_fill(multi, oracle, size, mode, eq):
    """The same pairs without the ring: the wave that finishes a pair walks its path at once, with all its lanes (walk_wave on the solo driver's stack)."""
    check(run_hip(multi, "dna", size, mode, eq), reference(oracle, "dna", size, mode, eq), "dna", size, mode)


@pytest.mark.parametrize("with_ring", [True, False])
@pytest.mark.parametrize("mode", SPECIAL)
def test_special_modes_in_the_slots(multi, monkeypatch, oracle, mode, with_ring):
    """LOCAL_START / FREE_QUERY_START_GAPS: the round-5 tb_step on the traceback waves, the one-lane walk behind the fill; LOCAL_START's zero mask keeps
    its own order."""
    if with_ring:
        monkeypatch.setenv("BA_FORCE_TB", "1")
        monkeypatch.setenv("BA_WGS_PER_CU", "1")
    for eq in (True, False):
        check(run_hip(multi, "flanked", (128, 512), mode, eq), reference(oracle, "flanked", (128, 512), mode, eq), "flanked", (128, 512), mode)


def test_k_small_keeps_the_cell_order(devlib, monkeypatch, oracle):
    """k_small's slot rectangles (the same record bit, the same walker code, the other order) and k_walk behind its fill."""
    monkeypatch.setenv("BA_FORCE_SMALL", "1")
    mode = ("trace", "x_drop")
    check(run_hip(devlib, "small", (32, 256), mode, True, kernel="k_small"), reference(oracle, "small", (32, 256), mode, True), "small", (32, 256), mode)


def test_sequence_prefetch_by_64_bit_offset(ring, monkeypatch, oracle):
    """BA_POOL64 forces the form a pool beyond 32 bits takes (F_POOL64: every step fetches its bytes by 64-bit offset): the same arrays as the 32-bit run."""
    key = ((128, 512), ("trace", "x_drop"), True)
    first = _first.get(key) or run_hip(ring, "dna", *key)
    monkeypatch.setenv("BA_POOL64", "1")
    second = run_hip(ring, "dna", *key)
    check(second, reference(oracle, "dna", *key), "dna", key[0], key[1])
    for k in ("score", "query_idx", "reference_idx", "cells", "cigar_len", "status"):
        assert np.array_equal(first[0][k], second[0][k]), k
    assert np.array_equal(first[1], second[1]) and np.array_equal(first[2], second[2])
