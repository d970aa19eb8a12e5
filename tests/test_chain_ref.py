"""The model of anchor-chain batches (tests/chain_ref.py) against the definitions it rests on, without a GPU: its spliced runs re-score to
its score, a chain of one anchor is a seed, and the generated sets meet every case the device splice has to handle."""
import numpy as np
import pytest

from block_aligner_amd import scores as S, verify
from tests import chain_ref as R
from tests.test_gpu_extend import SeedSet, composite

NUC = S.NucMatrix.new_simple(2, -3)
GAPS = (-5, -1)
SIZE = (32, 128)
X_DROP = 100


@pytest.fixture(scope="module")
def sets():
    return R.dna_sets()


@pytest.mark.parametrize("eq", [False, True])
def test_spliced_runs_rescore_to_the_score(oracle, sets, eq):
    piece = R.oracle_piece(oracle, NUC, GAPS, SIZE, X_DROP, True, eq)
    for name, cs in sets.items():
        for c, exp in enumerate(R.expected(piece, NUC, GAPS, cs, True, eq)):
            q, r = cs.q(c)[exp["q_start"]:exp["q_end"]], cs.r(c)[exp["r_start"]:exp["r_end"]]
            verify.check_cigar(exp["runs"], q, r, NUC, GAPS, exp["score"], len(q), len(r), what=f"{name} chain {c}")
            ops = {x & 15 for x in exp["runs"]}
            assert ops <= ({2, 3, 4, 5} if eq else {1, 4, 5})


@pytest.mark.parametrize("mode", [2, 3, 35])   # X_DROP, TRACE | X_DROP, TRACE | X_DROP | CIGAR_EQ
def test_one_anchor_is_a_seed(oracle, sets, mode):
    cs = sets["minus"].first_anchor_seeds()
    ss = SeedSet(cs.seqs, [c[0] for c in cs.chains], [c[1] for c in cs.chains], cs.q_anchor, cs.r_anchor, cs.anchor_len, cs.strand)
    trace, eq = bool(mode & 1), bool(mode & 32)
    piece = R.oracle_piece(oracle, NUC, GAPS, SIZE, X_DROP, trace, eq)
    for c, exp in enumerate(R.expected(piece, NUC, GAPS, cs, trace, eq)):
        assert exp == composite(oracle, NUC, GAPS, SIZE, X_DROP, mode, ss, c), c


def test_the_sets_are_not_vacuous(oracle, sets):
    counts = {}
    piece = R.oracle_piece(oracle, NUC, GAPS, SIZE, X_DROP, True, True)
    for cs in sets.values():
        R.expected(piece, NUC, GAPS, cs, True, True, counts)
    for k in ("gap_none", "gap_query_only", "gap_reference_only", "gap_aligned", "merges", "wide_groups", "chains_130"):
        assert counts[k] > 0, (k, counts)
    assert sum(len(cs) for cs in sets.values()) <= 3 * 300 and all(len(cs) <= 300 for cs in sets.values())
    assert any(cs.strand is not None and cs.strand.any() for cs in sets.values())
    assert any(s != s.upper() for cs in sets.values() for s in cs.seqs)   # lower case


@pytest.mark.parametrize("eq", [False, True])
def test_adjacent_exact_anchors_collapse_into_one_run(oracle, eq):
    cs = R.collapse_chain(130)
    assert len(cs.anchors(0)) >= 130
    counts = {}
    exp = R.expected(R.oracle_piece(oracle, NUC, GAPS, SIZE, X_DROP, True, eq), NUC, GAPS, cs, True, eq, counts)[0]
    # the ends' own runs, as the model takes them from the oracle
    q, r = cs.q(0), cs.r(0)
    s, t, _ = cs.anchors(0)[0]
    qe, re_ = cs.anchors(0)[-1][0] + 5, cs.anchors(0)[-1][1] + 5
    left = R.parse(oracle.align(NUC, q[:s][::-1], r[:t][::-1], GAPS, SIZE, X_DROP, ("trace", "x_drop"), cigar_eq=eq)["cigar"])[::-1]
    right = R.parse(oracle.align(NUC, q[qe:], r[re_:], GAPS, SIZE, X_DROP, ("trace", "x_drop"), cigar_eq=eq)["cigar"])
    match = 2 if eq else 1
    core = 130 * 5 + (left.pop()[0] if left and left[-1][1] == match else 0) + (right.pop(0)[0] if right and right[0][1] == match else 0)
    want = [n << 4 | op for n, op in left] + [core << 4 | match] + [n << 4 | op for n, op in right]
    assert exp["runs"] == want   # exactly one run apart from the ends
    assert counts["gap_none"] == 129 and counts["wide_groups"] == 1 and counts["chains_130"] == 1
