"""Minimizer seeding on the MI355X: sketch() and results() of every problem against the model of tests/seeding_ref.py, bit for bit, the
device-to-device hand-off into AnchorChainer, and the whole pipeline bytes -> Seeder -> AnchorChainer.from_seeder -> ChainBatchAligner against
the chain model over the oracle."""
import numpy as np
import pytest

from tests import chain_ref, chaining_ref, index_both_ref as B, index_ref as X, seeding_ref as S
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP, check as check_chain_batch
from tests.test_gpu_chaining import compare as compare_chainer
from tests.test_gpu_index import compare as compare_indexed
from tests.test_gpu_index_both import compare as compare_both

pytestmark = pytest.mark.gpu

_sets = {}       # the problem sets, built once
_expected = {}   # the model's results, computed once per (set, parameters)


def get_set(name, make):
    if name not in _sets:
        _sets[name] = make()
    return _sets[name]


def expected(name, P, ps):
    if (name, P) not in _expected:
        _expected[(name, P)] = ps.expected(P)
    return _expected[(name, P)]


def compare(sd, P, exps):
    """Every problem of the set, none left out: both sketches, positions and codes, and every hit."""
    assert sd.n == len(exps)
    sk = sd.sketch()
    first, q_hit, r_hit, hit_len, per = sd.results()
    assert per.tolist() == [len(e["q_hit"]) for e in exps]
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(e["q_hit"]) for e in exps])]).tolist()
    assert len(q_hit) == len(r_hit) == len(hit_len) == int(first[-1]) and (hit_len == P.k).all()
    assert sk["q_first"].tolist() == np.concatenate([[0], np.cumsum([len(e["q_pos"]) for e in exps])]).tolist()
    assert sk["r_first"].tolist() == np.concatenate([[0], np.cumsum([len(e["r_pos"]) for e in exps])]).tolist()
    assert len(sk["q_pos"]) == len(sk["q_code"]) == int(sk["q_first"][-1]) and len(sk["r_pos"]) == len(sk["r_code"]) == int(sk["r_first"][-1])
    for p, e in enumerate(exps):
        for side in "qr":
            a, b = int(sk[side + "_first"][p]), int(sk[side + "_first"][p + 1])
            assert np.array_equal(sk[side + "_pos"][a:b], e[side + "_pos"]), (p, side)
            assert np.array_equal(sk[side + "_code"][a:b], e[side + "_code"]), (p, side)
        a, b = int(first[p]), int(first[p + 1])
        assert np.array_equal(q_hit[a:b], e["q_hit"]), p
        assert np.array_equal(r_hit[a:b], e["r_hit"]), p
    c = sd.counts()
    assert (c["n_hits"], c["n_q_seeds"], c["n_r_seeds"]) == (len(q_hit), len(sk["q_pos"]), len(sk["r_pos"]))


def run(hip, name, P, ps):
    sd = hip.Seeder(*P, *ps.args())
    sd.run()
    compare(sd, P, expected(name, P, ps))
    sd.close()


def test_the_known_answers(hip):
    ps = S.ProblemSet([(S.KNOWN_Q, S.KNOWN_R, 0)])
    for occ, want in ((2, S.KNOWN_HITS_OCC2), (1, S.KNOWN_HITS_OCC1)):
        sd = hip.Seeder(5, 4, occ, *ps.args())
        sd.run()
        sk = sd.sketch()
        assert sk["q_pos"].tolist() == S.KNOWN_Q_SKETCH and sk["r_pos"].tolist() == S.KNOWN_R_SKETCH
        first, q, r, ln, per = sd.results()
        assert list(zip(q.tolist(), r.tolist())) == want and ln.tolist() == [5] * len(want) and first.tolist() == [0, len(want)] == [0, int(per[0])]
        sd.close()
    ps = S.ProblemSet([(S.KNOWN_Q_MINUS, S.KNOWN_R, 1)])
    sd = hip.Seeder(5, 3, 4, *ps.args())
    sd.run()
    assert sd.sketch()["q_pos"].tolist() == S.KNOWN_Q_MINUS_SKETCH
    first, q, r, ln, per = sd.results()
    assert list(zip(q.tolist(), r.tolist())) == S.KNOWN_HITS_MINUS
    sd.close()


@pytest.mark.parametrize("k", S.EDGE_K)
@pytest.mark.parametrize("w", S.EDGE_W)
def test_lengths_around_the_edges(hip, k, w):
    """No k-mer, one, one window, two; the chunk of 64 windows and its halo of k + w - 2 bytes; on either side; an empty side."""
    name = f"lengths_{k}_{w}"
    run(hip, name, S.Params(k, w, 4), get_set(name, lambda: S.lengths_set(k, w)))


@pytest.mark.parametrize("k, w", [(4, 1), (5, 4), (15, 10), (16, 64)])
def test_bytes_outside_acgt(hip, k, w):
    name = f"other_{k}_{w}"
    run(hip, name, S.Params(k, w, 8), get_set(name, lambda: S.other_bytes_set(k, w)))


@pytest.mark.parametrize("k, w", [(4, 1), (4, 7), (16, 64), (9, 2)])
def test_equal_hashes_in_every_window(hip, k, w):
    run(hip, "ties", S.Params(k, w, 1000), get_set("ties", S.tie_set))


@pytest.mark.parametrize("max_occ", [1, 3, 64])
def test_a_code_exactly_at_and_just_over_max_occ(hip, max_occ):
    name = f"occ_{max_occ}"
    run(hip, name, S.Params(6, 1, max_occ), get_set(name, lambda: S.occ_set(6, max_occ)))


def test_sort_paths(hip):
    """Queries of 1 .. 20000 entries: up to 8192 the network runs in LDS, above that in global memory (8193 and 20000, neither a power of two)."""
    ps = get_set("sort", S.sort_set)
    P = S.Params(15, 1, S.NO_CAP)
    exps = expected("sort", P, ps)
    assert [len(e["q_pos"]) for e in exps] == list(S.SORT_ENTRIES)
    sd = hip.Seeder(*P, *ps.args())
    sd.run()
    compare(sd, P, exps)
    sd.close()
    run(hip, "sort", P._replace(max_occ=1), ps)


def test_a_long_reference(hip):
    """70 kbp against a read of 500: the match's running offset crosses many steps."""
    ps = get_set("long", S.long_reference_set)
    for P in (S.Params(11, 1, S.NO_CAP), S.Params(8, 5, 50)):
        run(hip, "long", P, ps)


def test_2000_tiny_problems(hip):
    """More problems than the grids have waves, with empty sides among them."""
    run(hip, "tiny", S.Params(5, 3, 4), get_set("tiny", S.tiny_set))


def test_strands(hip):
    ps = get_set("strands", S.strand_set)
    run(hip, "strands", S.Params(8, 5, 4), ps)
    sd = hip.Seeder(8, 5, 4, *ps.args()[:5])   # strand NULL: every problem on the plus strand
    sd.run()
    plus = S.ProblemSet([(q, r, 0) for q, r, _ in ps.pairs])
    compare(sd, S.Params(8, 5, 4), plus.expected(S.Params(8, 5, 4)))
    sd.close()


def test_reload_with_a_smaller_set_and_back(hip):
    """Also the refusal of ba_chaining_create_seeded on a seeder that has not run: a seeder cannot be created without a device, so that
    rejection is checked here and not among the CPU rejections of tests/test_seeding_abi.py."""
    P = S.Params(6, 4, 4)
    ps, small = get_set("strands", S.strand_set), get_set("smaller", S.smaller_set)
    sd = hip.Seeder(*P, *ps.args())
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        hip.AnchorChainer.from_seeder(*chaining_ref.E2E_PARAMS, sd)
    sd.run()
    compare(sd, P, expected("strands", P, ps))
    sd.reload(*small.args())
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.sketch()
    sd.run()
    compare(sd, P, expected("smaller", P, small))
    sd.reload(*ps.args())
    sd.run()
    compare(sd, P, expected("strands", P, ps))
    with pytest.raises(RuntimeError, match="reload: .* sequence bytes exceed the batch's capacity"):
        sd.reload(*get_set("long", S.long_reference_set).args())
    with pytest.raises(RuntimeError, match="reload: .* problems exceed the batch's capacity"):
        sd.reload(*get_set("tiny", S.tiny_set).args())
    sd.close()


GROWTH_K, GROWTH_W, GROWTH_OCC = 11, 5, 16
# Reads of one length have about as many minimizers wherever they come from, so the generator's seed is one of those -- about one in three --
# whose reads from the reference have more than its unrelated ones, plain and canonical: 394 against 368, and 391 against 377. The test asserts it.
GROWTH_SEED = 52


def growth_reads(seed: int = GROWTH_SEED):
    """-> a reference of 2000 bases, 4 unrelated reads of 300, and 4 reads of 300 cut from the reference with 5 % of their bases
    substituted -- the same count and the same bytes --, the second and the fourth of them reverse-complemented."""
    rng = np.random.default_rng(seed)
    ref = S.dna(rng, 2000)
    unrelated = [S.dna(rng, 300) for _ in range(4)]
    cut = []
    for i in range(4):
        a = int(rng.integers(0, 2000 - 300 + 1))
        q = bytearray(ref[a:a + 300])
        for j in np.nonzero(rng.random(300) < 0.05)[0].tolist():
            q[j] = b"ACGT"[(b"ACGT".index(q[j]) + 1 + int(rng.integers(3))) % 4]   # another base
        cut.append(B.revcomp(bytes(q)) if i % 2 else bytes(q))
    return ref, unrelated, cut


def growth_kinds(hip):
    """Per kind of seeder -> (make(reads) -> (seeder, what to close with it), reload(seeder, reads), check(seeder, reads)): the reads that
    were reverse-complemented go on the minus strand where the kind takes a strand."""
    ref = get_set("growth", growth_reads)[0]
    strands = [0, 1, 0, 1]
    P = S.Params(GROWTH_K, GROWTH_W, GROWTH_OCC)
    XP = X.Params(GROWTH_K, GROWTH_W, GROWTH_OCC, X.NO_CAP)
    plain = lambda reads: S.ProblemSet([(q, ref, s) for q, s in zip(reads, strands)])   # noqa: E731
    listed = lambda reads: X.ReadSet(list(zip(reads, strands)))                          # noqa: E731

    def indexed(reads):
        ix = hip.RefIndex(GROWTH_K, GROWTH_W, ref)
        return hip.Seeder.indexed(ix, XP.max_occ, XP.max_ref_occ, *listed(reads).args()), ix

    def both(reads):
        ix = hip.RefIndex(GROWTH_K, GROWTH_W, ref, canonical=True)
        return hip.Seeder.indexed_both(ix, XP.max_occ, XP.max_ref_occ, *B.Reads(reads).args()), ix

    return dict(plain=(lambda reads: (hip.Seeder(*P, *plain(reads).args()), None), lambda sd, reads: sd.reload(*plain(reads).args()),
                       lambda sd, reads: compare(sd, P, plain(reads).expected(P))),
                indexed=(indexed, lambda sd, reads: sd.reload_indexed(*listed(reads).args()),
                         lambda sd, reads: compare_indexed(sd, GROWTH_K, listed(reads).expected(ref, XP))),
                both=(both, lambda sd, reads: sd.reload_indexed_both(*B.Reads(reads).args()),
                      lambda sd, reads: compare_both(sd, GROWTH_K, B.expected(reads, [ref], XP))))


@pytest.mark.parametrize("kind", ["plain", "indexed", "both"])
def test_growth_between_runs(hip, kind):
    """One handle from few seeds and close to no hits to many: the second run's buffers grow after its count passes, and the parameters of
    its emit passes are read again. Every entry of the sketch and every hit of both runs against the kind's model, bit for bit; the second
    run's times add up to what run() returned."""
    _, unrelated, cut = get_set("growth", growth_reads)
    make, reload, check = growth_kinds(hip)[kind]
    sd, ix = make(unrelated)
    sd.run()
    check(sd, unrelated)
    c = sd.counts()
    seeds, hits = c["n_q_seeds"] + c["n_r_seeds"], c["n_hits"]
    reload(sd, cut)
    ms = sd.run()
    check(sd, cut)
    c = sd.counts()
    assert c["n_q_seeds"] + c["n_r_seeds"] > seeds and c["n_hits"] > hits, (seeds, hits, c)   # (or nothing grew)
    t = sd.times()
    assert all(t[x] > 0 for x in ("sketch_ms", "sort_ms", "match_ms")), t
    assert ms == pytest.approx(t["sketch_ms"] + t["sort_ms"] + t["match_ms"], rel=1e-6), (ms, t)
    sd.close()
    if ix is not None:
        ix.close()


def test_over_the_limit(hip):
    """16 986 x 16 986 hits of one problem: run fails and names it; the same seeder then runs a small set."""
    ps = get_set("over", S.over_limit_set)
    P = S.Params(15, 1, S.NO_CAP)
    sd = hip.Seeder(*P, *ps.args())
    with pytest.raises(RuntimeError, match=rf"more than 2\^28 hits: problem 1 alone has {16986 * 16986}, .* lower max_occ"):
        sd.run()
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    small = get_set("smaller", S.smaller_set)
    sd.reload(*small.args())
    sd.run()
    compare(sd, P, expected("smaller", P, small))
    sd.close()


@pytest.mark.parametrize("name, make, P", [("lengths_15_16", lambda: S.lengths_set(15, 16), S.Params(15, 16, 4)),
                                           ("lengths_4_2", lambda: S.lengths_set(4, 2), S.Params(4, 2, 4)),
                                           ("tiny", S.tiny_set, S.Params(5, 3, 4))])
def test_the_hand_off(hip, name, make, P):
    """AnchorChainer.from_seeder against an AnchorChainer built from the seeder's host arrays, bit for bit, and both against the model."""
    ps = get_set(name, make)
    CP = chaining_ref.Params(4, 1, 1, 64, 400, 60, 4, 16, 1)
    sd = hip.Seeder(*P, *ps.args())
    sd.run()
    first, q, r, ln, _ = sd.results()
    a = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()   # (the chainer holds its own copy)
    b = hip.AnchorChainer(*CP, first, q, r, ln)
    assert a.n == b.n and a.n_anchors == b.n_anchors == len(q)
    a.run(); b.run()
    for x, y in zip(a.dp(), b.dp()):
        assert np.array_equal(x, y)
    ra, rb = a.results(), b.results()
    assert ra.keys() == rb.keys()
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), key
    exps = expected(name, P, ps)
    cps = chaining_ref.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exps])
    assert np.array_equal(cps.q_anchor, q) and np.array_equal(cps.r_anchor, r)
    compare_chainer(a, cps, cps.expected(CP))
    # the handle takes host arrays afterwards, as any chainer
    a.reload(first, q, r, ln)
    a.run()
    compare_chainer(a, cps, cps.expected(CP))
    a.close(); b.close()


def test_the_hand_off_with_the_seeder_alive_and_reused(hip):
    """The ordinary order: run() of the chainer straight after from_seeder, the seeder still open; then the seeder is reloaded with another
    set and run again while the chainer is in use: the chainer's hits are its own copy, complete when from_seeder returns."""
    P = S.Params(8, 5, 4)
    CP = chaining_ref.Params(4, 1, 1, 64, 400, 60, 4, 16, 1)
    ps, small = get_set("strands", S.strand_set), get_set("smaller", S.smaller_set)
    exps = expected("strands", P, ps)
    cps = chaining_ref.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exps])
    want = cps.expected(CP)
    sd = hip.Seeder(*P, *ps.args())
    sd.run()
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    ch.run()
    compare_chainer(ch, cps, want)
    sd.reload(*small.args())   # the seeder's buffers are rewritten ...
    sd.run()
    compare(sd, P, expected("smaller", P, small))
    ch.run()                   # ... and the chainer still holds the first set's hits
    compare_chainer(ch, cps, want)
    ch2 = hip.AnchorChainer.from_seeder(*CP, sd)   # a second chainer over the second set, both alive
    ch2.run()
    e2 = expected("smaller", P, small)
    cps2 = chaining_ref.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in e2])
    compare_chainer(ch2, cps2, cps2.expected(CP))
    ch.run()
    compare_chainer(ch, cps, want)
    sd.close(); ch.close(); ch2.close()


def test_an_empty_sequence_names_no_byte(hip):
    """The offset of an empty sequence is not read: far outside the pool it neither widens what is uploaded nor changes a result."""
    ps = S.ProblemSet([(S.KNOWN_Q, S.KNOWN_R, 0), (b"", S.KNOWN_R, 0), (S.KNOWN_Q_MINUS, b"", 1)])
    P = S.Params(5, 4, 2)
    exps = ps.expected(P)
    q_off, r_off = ps.q_off.copy(), ps.r_off.copy()
    q_off[1], r_off[2] = np.uint64(1) << np.uint64(60), np.uint64(0xfffffffffffffff0)
    sd = hip.Seeder(*P, ps.pool, q_off, ps.q_len, r_off, ps.r_len, ps.strand)
    sd.run()
    compare(sd, P, exps)
    sd.reload(ps.pool, q_off, ps.q_len, r_off, ps.r_len, ps.strand)   # (the capacity is the named bytes')
    sd.run()
    compare(sd, P, exps)
    sd.close()
    z = np.zeros(2, np.uint32)
    sd = hip.Seeder(*P, ps.pool, np.array([1 << 50, 7], np.uint64), z, np.array([3, 1 << 40], np.uint64), z)   # nothing but empty sequences
    sd.run()
    first, q, r, ln, per = sd.results()
    assert first.tolist() == [0, 0, 0] and len(q) == 0 and per.tolist() == [0, 0]
    sd.close()


def test_bytes_to_alignments(hip, oracle):
    """bytes -> Seeder -> from_seeder -> ChainBatchAligner on the minus-strand chain set: every read has a best chain, and every chain's
    result and runs equal the chain model over the oracle on the chainer's anchors."""
    cs = chain_ref.dna_sets()["minus"]
    args, pairs = S.chain_set_problems(cs)
    P, CP = S.PIPELINE_PARAMS, chaining_ref.E2E_PARAMS
    sd = hip.Seeder(*P, *args)
    sd.run()
    compare(sd, P, [S.hits(q, r, P, s) for q, r, s in pairs])
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()
    ch.run()
    res = ch.results()
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, mode, *ch.chain_batch_args(*args))
    assert cb.n == len(res["chain_problem"]) >= len(cs)
    assert sorted(set(res["chain_problem"][res["chain_rank"] == 0].tolist())) == list(range(len(cs)))   # every read has a best chain
    found = []   # the chains found, as a chain set over the same sequences
    for c, p in enumerate(res["chain_problem"].tolist()):
        lo, hi = int(res["anchor_first"][c]), int(res["anchor_first"][c + 1])
        anchors = list(zip(res["q_anchor"][lo:hi].tolist(), res["r_anchor"][lo:hi].tolist(), res["anchor_len"][lo:hi].tolist()))
        found.append((cs.chains[p][0], cs.chains[p][1], anchors, cs.chains[p][3]))
    check_chain_batch(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, mode, chain_ref.ChainSet(cs.seqs, found, True), cb=cb)
    cb.close()
    ch.close()
