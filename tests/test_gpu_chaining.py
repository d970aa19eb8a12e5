"""Anchor chaining on the MI355X: dp() and results() of every problem against the model of tests/chaining_ref.py, bit for bit, and the whole
pipeline raw hits -> AnchorChainer -> ChainBatchAligner against the chain model over the oracle."""
import numpy as np
import pytest

from tests import chain_ref, chaining_ref as R
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP, check as check_chain_batch

pytestmark = pytest.mark.gpu

_expected = {}   # the model's results, computed once per (set, parameters)


@pytest.fixture(scope="module")
def sets():
    return R.gpu_sets()


def expected(name, P, ps):
    k = (name, P)
    if k not in _expected:
        _expected[k] = ps.expected(P)
    return _expected[k]


def compare(ch, ps, exps):
    """Every problem of the set, none left out: f and pred of every anchor, and every chain with its anchors."""
    assert ch.n == len(ps) == len(exps)
    f, pred = ch.dp()
    res = ch.results()
    first = ps.anchor_first
    assert len(f) == len(pred) == int(first[-1])
    assert res["chains_per_problem"].tolist() == [len(e["chains"]) for e in exps]
    assert len(res["chain_problem"]) == sum(len(e["chains"]) for e in exps) and len(res["anchor_first"]) == len(res["chain_problem"]) + 1
    c = 0
    for p, e in enumerate(exps):
        a, b = int(first[p]), int(first[p + 1])
        assert f[a:b].tolist() == e["f"], p
        assert pred[a:b].tolist() == e["pred"], p
        for rank, (score, anchors) in enumerate(e["chains"]):
            assert (int(res["chain_problem"][c]), int(res["chain_rank"][c]), int(res["chain_score"][c])) == (p, rank, score), (p, rank)
            lo, hi = int(res["anchor_first"][c]), int(res["anchor_first"][c + 1])
            got = list(zip(res["q_anchor"][lo:hi].tolist(), res["r_anchor"][lo:hi].tolist(), res["anchor_len"][lo:hi].tolist(),
                           res["anchor_src"][lo:hi].tolist()))
            assert got == anchors, (p, rank)
            c += 1
    assert c == len(res["chain_problem"]) and int(res["anchor_first"][-1]) == len(res["q_anchor"])


def run(hip, name, P, ps):
    ch = hip.AnchorChainer(*P, *ps.args())
    ch.run()
    compare(ch, ps, expected(name, P, ps))
    ch.close()


def test_the_known_answer(hip, sets):
    P, ps = sets["known"]
    ch = hip.AnchorChainer(*P, *ps.args())
    ch.run()
    f, pred = ch.dp()
    assert f.tolist() == R.KNOWN_F and pred.tolist() == R.KNOWN_PRED
    res = ch.results()
    assert res["chain_score"].tolist() == [249, 32, 24] and res["chain_rank"].tolist() == [0, 1, 2] and res["anchor_first"].tolist() == [0, 6, 7, 8]
    got = list(zip(res["q_anchor"].tolist(), res["r_anchor"].tolist(), res["anchor_len"].tolist(), res["anchor_src"].tolist()))
    assert got == [a for _, an in R.KNOWN_CHAINS for a in an]
    ch.close()


def test_problems_of_0_1_63_64_65_anchors(hip, sets):
    run(hip, "sizes", *sets["sizes"])


def test_3000_anchors_wrap_the_ring(hip, sets):
    run(hip, "big", *sets["big"])


@pytest.mark.parametrize("lookback", R.LOOKBACKS)
def test_lookback(hip, sets, lookback):
    """1 .. 64: one pass over the lanes, part of them idle; 65 and 200: two and four passes, the last one partial."""
    for name in ("sizes", "big"):
        P, ps = sets[name]
        run(hip, name, P._replace(lookback=lookback), ps)


@pytest.mark.parametrize("lookback", R.WIDE_LOOKBACKS)
def test_the_widest_lookbacks(hip, sets, lookback):
    """Up to sixteen passes per anchor; from 961 on the ring has 2048 slots and a workgroup two waves; a predecessor 1001 anchors back is
    reached from 1001 on."""
    P, ps = sets["wide"]
    run(hip, "wide", P._replace(lookback=lookback), ps)


def test_2000_tiny_problems(hip, sets):
    """More problems than the fill has waves: every wave comes back to the work counter."""
    run(hip, "tiny", *sets["tiny"])


@pytest.mark.parametrize("max_chains", R.MAX_CHAINS)
def test_max_chains(hip, sets, max_chains):
    for name in ("sizes", "tiny"):
        P, ps = sets[name]
        run(hip, name, P._replace(max_chains=max_chains), ps)


def test_reload_with_a_smaller_set(hip, sets):
    P, ps = sets["sizes"]
    _, small = sets["smaller"]
    ch = hip.AnchorChainer(*P, *ps.args())
    ch.run()
    compare(ch, ps, expected("sizes", P, ps))
    ch.reload(*small.args())
    with pytest.raises(RuntimeError, match="ba_chaining_run has not been called"):
        ch.dp()
    ch.run()
    compare(ch, small, expected("smaller", P, small))
    ch.reload(*ps.args())   # and back: the first set still fits
    ch.run()
    compare(ch, ps, expected("sizes", P, ps))
    big = sets["big"][1]
    with pytest.raises(RuntimeError, match="reload: .* anchors exceed the batch's capacity"):
        ch.reload(*big.args())
    ch.close()


def test_raw_hits_to_alignments(hip, oracle):
    """The true anchors of a DNA chain set as overlapping 8-mers plus off-diagonal noise: the chainer's output goes into a chain batch as it
    stands, every chain's result and runs equal the chain model over the oracle on the chainer's anchors, and every read's best chain holds
    true shared positions only."""
    cs = chain_ref.dna_sets()["mixed"]
    ps, _ = R.e2e_problems(cs)
    P = R.E2E_PARAMS
    ch = hip.AnchorChainer(*P, *ps.args())
    ch.run()
    compare(ch, ps, ps.expected(P))
    res = ch.results()
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, mode, *ch.chain_batch_args(cs.pool, cs.q_off, cs.q_len, cs.r_off, cs.r_len))
    assert cb.n == len(res["chain_problem"]) >= len(cs)
    found = []   # the chains found, as a chain set over the same sequences
    for c, p in enumerate(res["chain_problem"].tolist()):
        lo, hi = int(res["anchor_first"][c]), int(res["anchor_first"][c + 1])
        anchors = list(zip(res["q_anchor"][lo:hi].tolist(), res["r_anchor"][lo:hi].tolist(), res["anchor_len"][lo:hi].tolist()))
        found.append((cs.chains[p][0], cs.chains[p][1], anchors, 0))
        if res["chain_rank"][c] == 0:
            true = R.true_positions(cs, p)
            assert all((qa + x, ra + x) in true for qa, ra, g in anchors for x in range(g)), p
    assert sorted(set(res["chain_problem"][res["chain_rank"] == 0].tolist())) == list(range(len(cs)))   # every read has a best chain
    check_chain_batch(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, mode, chain_ref.ChainSet(cs.seqs, found), cb=cb)
    cb.close()
    ch.close()
