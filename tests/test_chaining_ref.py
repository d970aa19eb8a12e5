"""The model of anchor chaining (tests/chaining_ref.py) against the rule it restates, without a GPU: the known answer of the rule, an
exhaustive search on small problems, the properties ba_chain_batch_create insists on, and that the sets of the GPU tests meet every case."""
import numpy as np
import pytest

from tests import chain_ref, chaining_ref as C


def test_the_known_answer():
    out = C.chain(C.KNOWN_PARAMS, C.KNOWN_Q, C.KNOWN_R, C.KNOWN_L)
    assert out["f"] == C.KNOWN_F
    assert out["pred"] == C.KNOWN_PRED
    assert out["chains"] == C.KNOWN_CHAINS
    assert out["gain"][6] == 5 and C.KNOWN_L[6] == 10   # anchor 6 is trimmed from 10 to 5
    ps = C.ProblemSet([(C.KNOWN_Q, C.KNOWN_R, C.KNOWN_L)])   # (the known answer is sorted as the rule asks)
    assert [x.tolist() for x in ps.problems[0]] == [C.KNOWN_Q, C.KNOWN_R, C.KNOWN_L]


def test_the_fill_finds_the_best_of_every_admissible_subsequence():
    rng = np.random.default_rng(11)
    for k in range(150):
        n = int(rng.integers(1, 11))
        ps = C.ProblemSet([C.random_problem(rng, n, span=80, noise=0.4)])
        q, r, L = ps.problems[0]
        P = C.Params(int(rng.integers(1, 6)), int(rng.integers(0, 4)), 0, n, 1 << 30, 1 << 30, 1, -(1 << 30), 1)
        f, _, _ = C.fill(P, q, r, L)
        assert max(f) == C.exhaustive_best(P, q, r, L), (k, q, r, L)


def test_output_chains_are_what_a_chain_batch_accepts():
    rng = np.random.default_rng(12)
    chains = 0
    for k in range(400):
        ps = C.ProblemSet([C.random_problem(rng, int(rng.integers(0, 60)), span=int(rng.integers(40, 400)), noise=float(rng.uniform(0, 0.8)))])
        P = C.Params(int(rng.integers(1, 6)), int(rng.integers(0, 3)), int(rng.integers(0, 3)), int(rng.integers(1, 70)), int(rng.integers(5, 300)),
                     int(rng.integers(0, 100)), int(rng.integers(1, 9)), int(rng.integers(-5, 80)), int(rng.integers(1, 4)))
        out = C.chain(P, *ps.problems[0])
        C.check_output(P, *ps.problems[0], out["chains"])
        assert len(out["chains"]) <= P.max_chains
        chains += len(out["chains"])
    assert chains > 400


def test_the_gpu_sets_meet_every_case():
    counts = {}
    sets = C.gpu_sets()
    for P, ps in sets.values():
        for prob, out in zip(ps.problems, ps.expected(P, counts)):
            C.check_output(P, *prob, out["chains"])
    for k in C.CASES:
        assert counts.get(k, 0) > 0, (k, counts)
    sizes = [len(p[0]) for p in sets["sizes"][1].problems]
    assert {0, 1, 63, 64, 65} <= set(sizes)
    assert max(len(p[0]) for p in sets["big"][1].problems) >= 3000 > 1024 + 64   # the ring wraps, several times
    assert len(sets["tiny"][1]) == 2000
    # the widest look-backs reach predecessors 601 and 1001 anchors back, the second one only from a look-back of 1001
    P, wide = sets["wide"]
    assert P.lookback == 1024
    for H, reached in ((960, {71, 601, 31}), (1000, {71, 601, 31}), (1001, {71, 601, 1001, 31}), (1024, {71, 601, 1001, 31})):
        pred = wide.expected(P._replace(lookback=H))[0]["pred"]
        assert {i - p for i, p in enumerate(pred) if p != C.NONE} == reached, H
    assert len(sets["smaller"][1]) < len(sets["sizes"][1]) and sets["smaller"][1].anchor_first[-1] < sets["sizes"][1].anchor_first[-1]   # fits a reload


def test_a_tie_goes_to_none_then_to_the_nearer_anchor():
    P = C.gpu_sets()["sizes"][0]
    counts = {}
    ps = C.ProblemSet([C.tie_problem()])
    out = ps.expected(P, counts)[0]
    assert (counts["tie_none"], counts["tie_nearer"]) == (1, 1)
    assert out["pred"] == [C.NONE, C.NONE, C.NONE, C.NONE, 3] and out["f"] == [24, 24, 24, 24, 30]


def test_rank_0_of_raw_hits_lies_on_true_shared_positions():
    """The end-to-end construction of tests/test_gpu_chaining.py: the true anchors of a chain set as overlapping 8-mers plus off-diagonal
    noise. For every read the best chain holds true positions only, and the chains found are what ba_chain_batch_create accepts."""
    cs = chain_ref.dna_sets()["mixed"]
    ps, noise = C.e2e_problems(cs)
    assert noise > 10 * len(cs)
    exps = ps.expected(C.E2E_PARAMS)
    trimmed = 0
    for c, (prob, out) in enumerate(zip(ps.problems, exps)):
        C.check_output(C.E2E_PARAMS, *prob, out["chains"])
        assert out["chains"], c
        true = C.true_positions(cs, c)
        for qa, ra, g, src in out["chains"][0][1]:
            assert all((qa + x, ra + x) in true for x in range(g)), (c, qa, ra, g)
            assert qa + g <= len(cs.q(c)) and ra + g <= len(cs.r(c))
            trimmed += g < int(prob[2][src])
    assert trimmed > len(cs)
    assert sum(len(o["chains"]) for o in exps) <= 300
