"""Read-level selection on the MI355X: every output of every candidate against the model of tests/select_ref.py, bit for bit, and the
hand-off from a chain batch that has run."""
import numpy as np
import pytest

from tests import chain_ref, chaining_ref, select_ref as R

pytestmark = pytest.mark.gpu

_expected = {}   # the model's results, computed once per (set, parameters, variant)


@pytest.fixture(scope="module")
def sets():
    return R.gpu_sets()


def expected(name, P, cs):
    k = (name, P)
    if k not in _expected:
        _expected[k] = cs.expected(P)
    return _expected[k]


def compare(res, exp, n, n_reads):
    """Every candidate and every read of the set, none left out."""
    assert len(res["cls"]) == n and len(res["kept_first"]) == n_reads + 1
    for k in ("cls", "mapq", "parent", "rank", "sub_score", "kept_first", "kept", "kept_per_read"):
        assert res[k].tolist() == exp[k], k


def run(hip, name, P, cs):
    sel = hip.Selector(*P, *cs.args())
    sel.run()
    compare(sel.results(), expected(name, P, cs), len(cs), cs.n_reads)
    sel.close()


def test_the_known_answer(hip, sets):
    cs = sets["known"]
    sel = hip.Selector(*R.KNOWN_PARAMS, *cs.args())
    sel.run()
    res = sel.results()
    for k, v in R.KNOWN_OUT.items():
        assert res[k].tolist() == v, k
    assert set(sel.times()) == {"group_ms", "mark_ms", "emit_ms"}
    sel.close()


def test_reads_of_0_1_2_63_64_65_200_1024_candidates(hip, sets):
    """The empty read, the wave boundary, a second and further chunks of heads, the cap; the caller's order is shuffled."""
    run(hip, "sizes", R.GPU_PARAMS, sets["sizes"])


def test_130_disjoint_spans_a_tie_read_and_an_excluded_read(hip, sets):
    """Three 64-head steps; one score for a whole read, so the index decides; a read whose candidates are all excluded."""
    run(hip, "special", R.GPU_PARAMS, sets["special"])


@pytest.mark.parametrize("max_secondary", R.MAX_SECONDARY)
def test_max_secondary(hip, sets, max_secondary):
    for name in ("sizes", "special"):
        run(hip, name, R.GPU_PARAMS._replace(max_secondary=max_secondary), sets[name])


@pytest.mark.parametrize("mask_permille", R.MASK_PERMILLE)
def test_mask_permille(hip, sets, mask_permille):
    for name in ("sizes", "special"):
        run(hip, name, R.GPU_PARAMS._replace(mask_permille=mask_permille), sets[name])


@pytest.mark.parametrize("sec_permille", R.SEC_PERMILLE)
def test_sec_permille(hip, sets, sec_permille):
    for name in ("sizes", "special"):
        run(hip, name, R.GPU_PARAMS._replace(sec_permille=sec_permille), sets[name])


def test_without_the_optional_arrays(hip, sets):
    """support NULL against support given (the sets hold values on both sides of full_support); strand and exclude NULL."""
    cs = sets["sizes"]
    run(hip, "sizes/no support", R.GPU_PARAMS, cs.replace(support=None))
    run(hip, "sizes/bare", R.GPU_PARAMS, cs.replace(strand=None, support=None, exclude=None))
    assert expected("sizes/no support", R.GPU_PARAMS, None)["mapq"] != expected("sizes", R.GPU_PARAMS, cs)["mapq"]


def test_3000_small_reads(hip, sets):
    """More reads than the marking has waves: every wave comes back to the work counter."""
    run(hip, "many", R.GPU_PARAMS, sets["many"])


def test_two_runs_give_equal_outputs(hip, sets):
    """The order in which the scatter fills a read's slice must not show."""
    cs = sets["sizes"]
    sel = hip.Selector(*R.GPU_PARAMS, *cs.args())
    sel.run()
    first = {k: v.copy() for k, v in sel.results().items()}
    sel.run()
    second = sel.results()
    for k, v in first.items():
        assert np.array_equal(v, second[k]), k
    compare(second, expected("sizes", R.GPU_PARAMS, cs), len(cs), cs.n_reads)
    sel.close()


def test_reload_with_a_smaller_set_and_back(hip, sets):
    P = R.GPU_PARAMS
    cs, small = sets["sizes"], sets["smaller"]
    sel = hip.Selector(*P, *cs.args())
    with pytest.raises(RuntimeError, match="ba_select_run has not been called"):
        sel.results()
    sel.run()
    compare(sel.results(), expected("sizes", P, cs), len(cs), cs.n_reads)
    sel.reload(*small.args())
    with pytest.raises(RuntimeError, match="ba_select_run has not been called"):
        sel.results()
    sel.run()
    compare(sel.results(), expected("smaller", P, small), len(small), small.n_reads)
    sel.reload(*cs.args())   # and back: the first set still fits
    sel.run()
    compare(sel.results(), expected("sizes", P, cs), len(cs), cs.n_reads)
    with pytest.raises(RuntimeError, match="reload: .* candidates exceed the batch's capacity"):
        sel.reload(*sets["many"].args())
    with pytest.raises(RuntimeError, match="reload: .* reads exceed the batch's capacity"):
        sel.reload(*small.replace(n_reads=cs.n_reads + 1).args())
    sel.run()   # a refused reload leaves the set loaded
    compare(sel.results(), expected("sizes", P, cs), len(cs), cs.n_reads)
    sel.close()


# ------------------------------------------------------------------ from a chain batch
def both_strands(cs, k=8, cap=40):
    """Every read of a plus-strand chain set listed on both strands -> (ProblemSet, q_off, q_len, r_off, r_len, strand), problem 2c the
    raw hits of chain c's true anchors, problem 2c + 1 the read's reverse complement against the same reference: at most `cap` of its
    exact k-mer matches, which is all a mapper finds on the wrong strand."""
    plus, _ = chaining_ref.e2e_problems(cs)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    problems = []
    for c in range(len(cs)):
        q, r = cs.q(c).upper().translate(comp)[::-1], cs.r(c).upper()
        where = {}
        for j in range(len(r) - k + 1):
            where.setdefault(r[j:j + k], []).append(j)
        hits = [(i, j) for i in range(len(q) - k + 1) for j in where.get(q[i:i + k], ())][:cap]
        problems += [plus.problems[c], ([h[0] for h in hits], [h[1] for h in hits], [k] * len(hits))]
    twice = lambda x: np.repeat(x, 2)
    return (chaining_ref.ProblemSet(problems), twice(cs.q_off), twice(cs.q_len), twice(cs.r_off), twice(cs.r_len),
            np.tile(np.array([0, 1], np.uint8), len(cs)))


@pytest.fixture(scope="module")
def mapped(hip):
    """The "mixed" DNA chain set through AnchorChainer and ChainBatchAligner, as tests/test_gpu_chaining.py runs it, on both strands."""
    from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP
    cs = chain_ref.dna_sets()["mixed"]
    assert cs.strand is None
    ps, q_off, q_len, r_off, r_len, strand = both_strands(cs)
    ch = hip.AnchorChainer(*chaining_ref.E2E_PARAMS, *ps.args())
    ch.run()
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ,
                               *ch.chain_batch_args(cs.pool, q_off, q_len, r_off, r_len, strand))
    yield cs, ch, cb, q_len, strand
    cb.close()
    ch.close()


def test_from_a_chain_batch(hip, mapped):
    cs, ch, cb, q_len, strand = mapped
    P = R.GPU_PARAMS
    chains = ch.results()
    cp = chains["chain_problem"]
    read_of_chain = (cp // 2).astype(np.uint32)
    support = np.diff(chains["anchor_first"].astype(np.int64)).astype(np.uint32)
    with pytest.raises(RuntimeError, match=r"the batch has not finished a run \(ba_chain_batch_run\)"):
        hip.Selector.from_chain_batch(*P, cb, read_of_chain, support, len(cs))
    cb.run()
    sel = hip.Selector.from_chain_batch(*P, cb, read_of_chain, support, len(cs))
    res = cb.results()
    assert (cp % 2 == 1).any()   # the wrong strand gave candidates too
    failed = (res["status"] & hip.STATS_FAILED_BITS) != 0
    exp = R.select(P, read_of_chain, res["score"], res["q_start"], res["q_end"], q_len[cp], strand[cp], support, failed.astype(np.uint8), len(cs))
    # the selector holds a copy: what becomes of the batch afterwards does not reach it
    cb.reload(*ch.chain_batch_args(cs.pool, np.repeat(cs.q_off, 2), q_len, np.repeat(cs.r_off, 2), np.repeat(cs.r_len, 2), strand))
    with pytest.raises(RuntimeError, match=r"the batch has not finished a run \(ba_chain_batch_run\)"):
        hip.Selector.from_chain_batch(*P, cb, read_of_chain, support, len(cs))
    sel.run()
    got = sel.results()
    compare(got, exp, cb.n, len(cs))
    for r in range(len(cs)):   # every read has a primary, on its true strand
        prim = [c for c in np.nonzero(read_of_chain == r)[0].tolist() if got["cls"][c] == hip.SEL_PRIMARY]
        assert len(prim) == 1 and strand[cp[prim[0]]] == 0, r
    with pytest.raises(RuntimeError, match="ba_select_create_chained"):
        sel.reload(read_of_chain, res["score"], res["q_start"], res["q_end"], q_len[cp])
    # a failed chain cannot be provoked: the host path's exclude does what a failed status does
    ex = np.zeros(cb.n, np.uint8)
    ex[got["kept"][0]] = 1
    host = hip.Selector(*P, read_of_chain, res["score"], res["q_start"], res["q_end"], q_len[cp], strand[cp], support, ex, len(cs))
    host.run()
    out = host.results()
    compare(out, R.select(P, read_of_chain, res["score"], res["q_start"], res["q_end"], q_len[cp], strand[cp], support, ex, len(cs)), cb.n, len(cs))
    assert out["cls"][got["kept"][0]] == hip.SEL_EXCLUDED
    host.close()
    sel.close()


def test_from_chains_prunes_before_the_alignment(hip, mapped):
    cs, ch, cb, q_len, strand = mapped
    P = R.GPU_PARAMS
    chains = ch.results()
    read_of_problem = np.arange(2 * len(cs)) // 2
    sel = hip.Selector.from_chains(*P, ch, read_of_problem, q_len, strand)
    sel.run()
    cp, first = chains["chain_problem"], chains["anchor_first"].astype(np.int64)
    last = first[1:] - 1
    exp = R.select(P, read_of_problem[cp], chains["chain_score"], chains["q_anchor"][first[:-1]], chains["q_anchor"][last] + chains["anchor_len"][last],
                   q_len[cp], strand[cp], np.diff(first), None, len(cs))
    compare(sel.results(), exp, len(cp), len(cs))
    assert 0 < len(sel.results()["kept"]) < len(cp)
    sel.close()
