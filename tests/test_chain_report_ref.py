"""The combine rule of chain statistics (k_stats_chain; INTEGRATION.md, "Statistics and strings of a chain") without a GPU: per-element
ref_stats records, added and maximised, equal ref_stats over the chain's spliced runs -- for every chain of the sets the GPU tests run --,
and those sets contain every case the rule has."""
import numpy as np
import pytest

from tests import chain_ref as R, chain_report_ref as M
from tests.test_gpu_stats import FIELDS


def _sets():
    out = [(name, cs, M.DNA) for name, cs in R.dna_sets().items()]
    out += [("protein", M.protein_set(), M.PROTEIN), ("bytes", M.bytes_set(), M.BYTES), ("boundary", M.boundary_set(), M.DNA),
            ("no aligned gap", M.no_aligned_gap_set(), M.DNA)]
    return out


@pytest.fixture(scope="module")
def sets():
    return _sets()


def check_set(oracle, cs, cfg, eq, counts, what):
    m, gaps = cfg["m"], cfg["gaps"]
    piece = R.oracle_piece(oracle, m, gaps, cfg["size"], cfg["x_drop"], True, eq)
    exps = R.expected(piece, m, gaps, cs, True, eq, counts)
    for c, exp in enumerate(exps):
        q, r = cs.q(c), cs.r(c)
        records, start = M.element_records(piece, m, gaps, q, r, cs.anchors(c), eq, counts)
        got, want = M.combine(records, start), M.whole_record(exp, m, gaps, q, r)
        assert got == want, (what, c, got, want)
        assert (want["q_start"], want["r_start"], want["path_score"]) == (exp["q_start"], exp["r_start"], exp["score"]), (what, c)
        assert want["matches"] + want["mismatches"] + want["ins"] + want["del"] == want["columns"]
        assert len(records) <= 2 * len(cs.anchors(c)) + 1
        if cs.strand is not None and cs.chains[c][3] and cs.seqs[cs.chains[c][0]] != cs.seqs[cs.chains[c][0]].upper():
            counts["minus_lower"] = counts.get("minus_lower", 0) + 1


@pytest.mark.parametrize("eq", [False, True])
def test_the_combine_equals_the_record_of_the_spliced_runs(oracle, sets, eq):
    counts = {}
    for name, cs, cfg in sets:
        check_set(oracle, cs, cfg, eq, counts, name)
    for k in ("gap_none", "gap_query_only", "gap_reference_only", "gap_aligned", "left_end", "no_left_end", "right_end", "no_right_end", "minus_lower",
              "mismatching_anchor", "wide_groups", "chains_130"):
        assert counts.get(k, 0) > 0, (k, counts)


def test_the_dna_sets_alone_cover_the_cases(oracle):
    """The first GPU test runs dna_sets() only: they hold every gap kind, chains with and without each end, a lower-case read on the minus
    strand, a mismatching anchor and a merge across three or more elements between them."""
    counts = {}
    for name, cs in R.dna_sets().items():
        check_set(oracle, cs, M.DNA, True, counts, name)
    for k in ("gap_none", "gap_query_only", "gap_reference_only", "gap_aligned", "left_end", "no_left_end", "right_end", "no_right_end", "minus_lower",
              "mismatching_anchor", "wide_groups"):
        assert counts.get(k, 0) > 0, (k, counts)


def test_a_failed_chain_has_a_zero_record():
    """The rule for a chain with a STATS_FAILED bit, as the reference states it: all zeros (and empty text, tests/text_ref.py)."""
    from tests import text_ref as T
    exp = dict(runs=[5 << 4 | 1], q_end=5, r_end=5, status=8)
    assert M.whole_record(exp, M.NUC, (-5, -1), b"ACGTA", b"ACGTA") == dict.fromkeys(FIELDS, 0)
    assert T.render(T.CIGAR, exp["runs"], b"ACGTA", b"ACGTA", 0, 0, True, 8) == ""


def test_the_boundary_set_has_the_element_counts():
    cs = M.boundary_set()
    ks = [len(cs.anchors(c)) for c in range(len(cs))]
    assert ks == list(M.BOUNDARY_K) + [1, 130]
    assert {2 * k + 1 for k in ks} >= {63, 65, 127, 129, 131, 261}
    q, r, an = cs.q(len(M.BOUNDARY_K)), cs.r(len(M.BOUNDARY_K)), cs.anchors(len(M.BOUNDARY_K))
    (qa, ra, L), = an
    assert L == 300 and sum(x != y for x, y in zip(q[qa:qa + L], r[ra:ra + L])) == 3
    kinds = set()
    for c in range(len(M.BOUNDARY_K)):   # the gaps are mixed
        a = cs.anchors(c)
        for (q0, r0, l0), (q1, r1, _) in zip(a, a[1:]):
            kinds.add((q1 > q0 + l0, r1 > r0 + l0))
    assert len(kinds) == 4
    assert np.all(cs.q_len < 12000)
