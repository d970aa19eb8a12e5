"""Anchor-chain batches on the MI355X: every field and every run of every chain against the model of tests/chain_ref.py over the oracle --
the ends and the gaps aligned on host-cut slices, the anchors scored and everything spliced in Python."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import chain_ref as R

pytestmark = pytest.mark.gpu

NUC = S.NucMatrix.new_simple(2, -3)
DNA_GAPS = (-5, -1)
X_DROP = 100
_expected = {}   # the model's results are computed once per (set, configuration) and shared


@pytest.fixture(scope="module")
def sets():
    return R.dna_sets()


def flags_of(hip, mode):
    f = 0
    for name in mode.split("|"):
        f |= getattr(hip, name)
    return f


def expected(oracle, m, gaps, size, x_drop, mode, cs, key=None):
    trace, eq = bool(mode & 1), bool(mode & 32)
    k = None if key is None else (key, size, x_drop, trace, eq)
    if k is not None and k in _expected:
        return _expected[k]
    piece = R.oracle_piece(oracle, m, gaps, size, x_drop, trace, eq)
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 4)) as ex:
        exps = list(ex.map(lambda c: R.chain_result(piece, m, gaps, cs.q(c), cs.r(c), cs.anchors(c), trace, eq), range(len(cs))))
    if k is not None:
        _expected[k] = exps
    return exps


def check(hip, oracle, m, gaps, size, x_drop, mode, cs, cb=None, key=None):
    """Every chain of the set, none left out: the results, status 0, and with TRACE the runs."""
    assert len(cs) <= 300
    own = cb is None
    if own:
        cb = hip.ChainBatchAligner(m, gaps, size, x_drop, mode, *cs.args(), strand=cs.strand)
    cb.run()
    res = cb.results()
    runs = off = None
    if mode & 1:
        runs, off = cb.cigars(res["cigar_len"])
    exps = expected(oracle, m, gaps, size, x_drop, mode, cs, key)
    for c, exp in enumerate(exps):
        got = {k: int(res[k][c]) for k in R.FIELDS}
        assert got == {k: exp[k] for k in R.FIELDS}, (c, got, exp)
        assert got["status"] == 0
        if mode & 1:
            mine = [int(x) for x in runs[int(off[c]):int(off[c + 1])]]
            assert mine == exp["runs"], (c, hip.runs_to_string(mine), hip.runs_to_string(exp["runs"]))
        else:
            assert int(res["cigar_len"][c]) == 0
    times = cb.times()
    if own:
        cb.close()
    return res, times


@pytest.mark.parametrize("size", [(32, 128), (32, 256)])
@pytest.mark.parametrize("mode", ["X_DROP", "TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
@pytest.mark.parametrize("name", ["mixed", "dense"])
def test_dna_parity(hip, oracle, sets, name, mode, size):
    """mixed: reads of 200 .. 3000 bp with every kind of gap; dense: chains of more than 130 elements (several chunks of 64 per wave)."""
    check(hip, oracle, NUC, DNA_GAPS, size, X_DROP, flags_of(hip, mode), sets[name], key=name)


@pytest.mark.parametrize("mode", ["X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_minus_strand(hip, oracle, sets, mode):
    cs = sets["minus"]
    assert cs.strand.sum() > 20
    check(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, flags_of(hip, mode), cs, key="minus")


@pytest.mark.parametrize("mode", ["TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_protein(hip, oracle, mode):
    cs = R.make_set(np.random.default_rng(7), 80, lo=200, hi=1200, alphabet=synth.AMINO, spacing=(10, 80), anchor=(4, 12), edit_div=6)
    check(hip, oracle, S.static_matrix("BLOSUM62"), (-11, -1), (32, 128), 50, flags_of(hip, mode), cs)


@pytest.mark.parametrize("mode", ["TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_bytes(hip, oracle, mode):
    """A ByteMatrix scores its padding byte as an ordinary mismatch, so an X-drop end may stop inside the padding, which the reference's
    traceback refuses (no traced X-drop test of this suite uses one): the chains of this set have no ends, the anchors and every kind of gap."""
    cs = R.without_ends(R.make_set(np.random.default_rng(8), 80, lo=200, hi=1200, alphabet=np.arange(250, 256, dtype=np.uint8), lower=False))
    check(hip, oracle, S.ByteMatrix.new_simple(3, -2), (-4, -2), (32, 256), 40, flags_of(hip, mode), cs)


@pytest.mark.parametrize("mode", ["X_DROP", "TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_one_anchor_equals_the_extension_batch(hip, sets, mode):
    """K = 1 is a seed: every array of ExtendBatchAligner on the same seeds, bit for bit."""
    flags = flags_of(hip, mode)
    cs = sets["minus"].first_anchor_seeds()
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, flags, *cs.args(), strand=cs.strand)
    eb = hip.ExtendBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, flags, cs.pool, cs.q_off, cs.q_len, cs.r_off, cs.r_len, cs.q_anchor, cs.r_anchor,
                                cs.anchor_len, strand=cs.strand)
    cb.run(); eb.run()
    got, want = cb.results(), eb.results()
    assert list(got) == list(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert want["cells"].any() and not want["status"].any()
    if flags & 1:
        (r1, o1), (r2, o2) = cb.cigars(got["cigar_len"]), eb.cigars(want["cigar_len"])
        assert np.array_equal(r1, r2) and np.array_equal(o1, o2) and len(r2)
    assert cb.times()["gaps_ms"] == 0
    cb.close(); eb.close()


@pytest.mark.parametrize("mode", ["TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_adjacent_exact_anchors_collapse(hip, oracle, mode):
    """130 adjacent exact anchors with nothing between them: one run apart from the ends, a merge group across three chunks of 64 elements."""
    cs = R.collapse_chain(130)
    res, times = check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, flags_of(hip, mode), cs)
    assert times["gaps_ms"] == 0   # (129 empty gaps: no gap batch)


def wide_gap_chain(eq: bool, seed=5):
    """Three anchors, two gaps of 600 reference bases; the read differs every few bases -- by a substitution (eq: = and X runs alternate) or
    by a missing base (M and D runs alternate) --, so that each gap piece has more than 64 runs."""
    rng = np.random.default_rng(seed)
    anchors, read, ref, L = [], [], [], 20
    for k in range(3):
        a = synth.rand_str(rng, L, synth.DNA)
        anchors.append((sum(map(len, read)), sum(map(len, ref)), L))
        read.append(a); ref.append(a)
        if k < 2:
            g = synth.rand_str(rng, 600, synth.DNA)
            ref.append(g)
            if eq:
                h = g.copy()
                h[3::7] = np.frombuffer(g.tobytes().translate(bytes.maketrans(b"ACGT", b"CGTA")), np.uint8)[3::7]
                read.append(h)
            else:
                read.append(np.delete(g, np.arange(4, 600, 8)))
    return R.ChainSet([np.concatenate(read).tobytes(), np.concatenate(ref).tobytes()], [(0, 1, anchors, 0)])


@pytest.mark.parametrize("mode", ["TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_gap_pieces_of_more_than_64_runs(hip, oracle, mode):
    flags = flags_of(hip, mode)
    eq = bool(flags & 32)
    cs = wide_gap_chain(eq)
    q, r, an = cs.q(0), cs.r(0), cs.anchors(0)
    for k in range(2):   # every gap piece of the chain, as the oracle aligns it
        g = oracle.align(NUC, q[an[k][0] + an[k][2]:an[k + 1][0]], r[an[k][1] + an[k][2]:an[k + 1][1]], DNA_GAPS, (32, 128), 0, ("trace",), cigar_eq=eq)
        assert len(R.parse(g["cigar"])) > 64
    check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, flags, cs)


def test_no_aligned_gap_means_no_gap_batch(hip, oracle):
    cs = R.make_set(np.random.default_rng(9), 60, lo=200, hi=800, p_adjacent=0.4, p_query_only=0.3, p_reference_only=0.31)
    counts = {}
    R.expected(R.oracle_piece(oracle, NUC, DNA_GAPS, (32, 128), X_DROP, True, True), NUC, DNA_GAPS, cs, True, True, counts)
    assert counts["gap_aligned"] == 0 and counts["gap_none"] and counts["gap_query_only"] and counts["gap_reference_only"]
    for mode in ("TRACE|X_DROP|CIGAR_EQ", "X_DROP"):
        res, times = check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, flags_of(hip, mode), cs)
        assert times["gaps_ms"] == 0 and times["ends_ms"] > 0


def test_no_end_means_no_ends_batch(hip, oracle, sets):
    """Every chain starts with its first anchor and ends with its last one: nothing to extend."""
    cs = R.without_ends(sets["mixed"], 60)
    for mode in ("TRACE|X_DROP", "X_DROP"):
        res, times = check(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, flags_of(hip, mode), cs)
        assert times["ends_ms"] == 0 and times["gaps_ms"] > 0
        assert not res["left_score"].any() and not res["right_score"].any() and not res["q_start"].any()


def test_reload_to_a_smaller_set_and_back(hip, oracle, sets):
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    big = sets["mixed"]
    small = big.subset(range(10, 50))
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 128), X_DROP, mode, *big.args(), strand=big.strand)
    with pytest.raises(RuntimeError, match="ba_chain_batch_run has not been called"):
        cb.results()
    with pytest.raises(RuntimeError, match="ba_chain_batch_run has not been called"):
        cb.cigars(np.zeros(len(big), np.uint32))
    res, _ = check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, mode, big, cb=cb, key="mixed")
    total = int(res["cigar_len"].sum())
    short = np.zeros(total - 1, np.uint32)
    assert hip.lib().ba_chain_batch_cigars(cb._h, short.ctypes.data, short.size) != 0
    assert f"cigar buffer too small: need {total} entries" in hip.last_error()
    cb.reload(*small.args(), strand=small.strand)
    with pytest.raises(RuntimeError, match="ba_chain_batch_run has not been called"):
        cb.results()
    check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, mode, small, cb=cb)
    cb.reload(*big.args(), strand=big.strand)
    check(hip, oracle, NUC, DNA_GAPS, (32, 128), X_DROP, mode, big, cb=cb, key="mixed")
    cb.close()
