"""The reference index on the MI355X: RefIndex.entries() and the results of an indexed Seeder against the models of tests/index_ref.py, bit
for bit; the plain Seeder over the same reads with r the whole reference; the lifecycle; and the whole path bytes of one reference + bytes
of many reads -> Seeder.indexed -> AnchorChainer.from_seeder -> candidate windows -> ChainBatchAligner against the chain model over the
oracle, with every read placed where it was drawn from."""
import numpy as np
import pytest

from tests import chain_ref, index_ref as X, seeding_ref as S
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP, check as check_chain_batch

pytestmark = pytest.mark.gpu

_mapping = {}   # the read set of the whole path and the model's hits, built once


def compare(sd, k, exps):
    """Every problem, none left out: the query's sketch, no reference entries, and every hit."""
    assert sd.n == len(exps)
    sk = sd.sketch()
    first, q_hit, r_hit, hit_len, per = sd.results()
    assert per.tolist() == [len(e["q_hit"]) for e in exps]
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(e["q_hit"]) for e in exps])]).tolist()
    assert len(q_hit) == len(r_hit) == len(hit_len) == int(first[-1]) and (hit_len == k).all()
    assert sk["q_first"].tolist() == np.concatenate([[0], np.cumsum([len(e["q_pos"]) for e in exps])]).tolist()
    assert sk["r_first"].tolist() == [0] * (sd.n + 1) and len(sk["r_pos"]) == len(sk["r_code"]) == 0
    for p, e in enumerate(exps):
        a, b = int(sk["q_first"][p]), int(sk["q_first"][p + 1])
        assert np.array_equal(sk["q_pos"][a:b], e["q_pos"]) and np.array_equal(sk["q_code"][a:b], e["q_code"]), p
        a, b = int(first[p]), int(first[p + 1])
        assert np.array_equal(q_hit[a:b], e["q_hit"]), p
        assert np.array_equal(r_hit[a:b], e["r_hit"]), p
    c = sd.counts()
    assert (c["n_hits"], c["n_q_seeds"], c["n_r_seeds"]) == (len(q_hit), len(sk["q_pos"]), 0)


def run(hip, ref, rs, P):
    ix = hip.RefIndex(P.k, P.w, ref)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *rs.args())
    sd.run()
    exps = rs.expected(ref, P)
    compare(sd, P.k, exps)
    sd.close(); ix.close()
    return exps


@pytest.mark.parametrize("k, w", X.SEAM_KW)
def test_the_sketch_across_the_seams_of_its_spans(hip, k, w):
    """entries() and longest_run against the model's sketch sorted by (code, pos): window counts around one and two spans, runs of A and
    of N across a seam, the all-T 16-mer (the last prefix of the table), and references of fewer k-mers than one window."""
    for name, ref in X.seam_references(k, w).items():
        code, pos, longest = X.entries(ref, k, w)
        ix = hip.RefIndex(k, w, ref)
        c = ix.counts()
        assert (c["k"], c["w"], c["ref_len"]) == (k, w, len(ref)), name
        assert (c["n_entries"], c["longest_run"]) == (len(code), longest), name
        got_code, got_pos = ix.entries()
        assert np.array_equal(got_code, code) and np.array_equal(got_pos, pos), name
        t = ix.times()
        assert set(t) == {"sketch_ms", "sort_ms", "table_ms"} and all(v >= 0 for v in t.values())
        ix.close()
    if k == 16:
        assert 0xffffffff in X.entries(X.seam_references(k, w)["all_t"], k, w)[0]   # the case is what it says


def test_the_known_answers_on_both_strands(hip):
    rs = X.known_reads()
    for k, w, occ in ((5, 4, 2), (5, 4, 1), (5, 3, 4)):
        exps = run(hip, S.KNOWN_R, rs, X.Params(k, w, occ, X.NO_CAP))
        assert [len(e["q_hit"]) for e in exps[4:]] == [0, 0, 0]   # no valid k-mer, empty, no hit
    P = X.Params(5, 4, 2, X.NO_CAP)
    e = rs.expected(S.KNOWN_R, P)
    assert list(zip(e[0]["q_hit"].tolist(), e[0]["r_hit"].tolist())) == S.KNOWN_HITS_OCC2
    run(hip, S.KNOWN_R, rs, P._replace(max_ref_occ=1))   # TTGCA is twice in the reference's sketch: its hits go


@pytest.mark.parametrize("max_occ, max_ref_occ", [(1, 1), (2, 3), (64, 2)])
def test_codes_exactly_at_and_just_over_either_cap(hip, max_occ, max_ref_occ):
    for k in (4, 13, 16):
        ref, rs = X.occ_case(k, max_occ, max_ref_occ)
        exps = run(hip, ref, rs, X.Params(k, 1, max_occ, max_ref_occ))
        if k > 4:   # (with k = 4 the unrelated stretches share k-mers)
            assert len(exps[0]["q_hit"]) == max_occ * max_ref_occ


@pytest.mark.parametrize("k, w", [(4, 1), (11, 5), (16, 64)])
def test_without_a_reference_cap_the_hits_equal_the_plain_seeders(hip, k, w):
    """results() of the indexed seeder and of a plain Seeder over the same reads, every problem's r the whole reference."""
    rng = np.random.default_rng(61)
    ref = S.dna(rng, 6000)
    reads = [(S.oriented(S.mutate(rng, ref[a:a + n], 0.05), s), s) for a, n, s in ((100, 700, 0), (2500, 900, 1), (5000, 1000, 0), (0, 300, 1))]
    rs = X.ReadSet(reads + [(S.dna(rng, 200), 0), (b"", 1)])
    ix = hip.RefIndex(k, w, ref)
    for max_occ in (3, X.NO_CAP):
        a = hip.Seeder.indexed(ix, max_occ, X.NO_CAP, *rs.args())
        b = hip.Seeder(k, w, max_occ, *rs.plain_args(ref))
        a.run(); b.run()
        for x, y in zip(a.results(), b.results()):
            assert np.array_equal(x, y)
        assert a.n_hits > 0
        t = a.times()
        assert set(t) == {"sketch_ms", "sort_ms", "match_ms"} and all(v >= 0 for v in t.values())
        a.close(); b.close()
    ix.close()


@pytest.mark.parametrize("extra", [0, 1])
def test_the_hit_sort_at_and_over_what_fits_in_lds(hip, extra):
    """Problems with 0, 1 and 2 hits, and one with SORT_LDS + extra: 128 x 64 from one code and `extra` unique shared k-mers."""
    k = 12
    ref, rs = X.hit_sort_case(extra, k)
    exps = run(hip, ref, rs, X.Params(k, 1, 64, 128))
    assert [len(e["q_hit"]) for e in exps] == [0, 1, X.SORT_LDS + extra, 2, X.SORT_LDS + extra]
    exps = run(hip, ref, rs, X.Params(k, 1, 64, 127))   # one under: the big code is over the reference cap
    assert [len(e["q_hit"]) for e in exps] == [0, 1, extra, 2, extra]


def test_lifecycle(hip):
    P = X.Params(5, 4, 2, X.NO_CAP)
    rs = X.known_reads()
    ix = hip.RefIndex(P.k, P.w, S.KNOWN_R)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *rs.args())
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    ix.close()   # the seeder shares the index's buffers
    sd.run()
    compare(sd, P.k, rs.expected(S.KNOWN_R, P))
    small = X.ReadSet(rs.reads[2:4])
    sd.reload_indexed(*small.args())
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    sd.run()
    compare(sd, P.k, small.expected(S.KNOWN_R, P))
    with pytest.raises(RuntimeError, match="ba_seeding_reload_indexed"):
        sd.reload(*small.plain_args(S.KNOWN_R))
    sd.reload_indexed(*rs.args())   # back to the first set: its capacity
    sd.run()
    compare(sd, P.k, rs.expected(S.KNOWN_R, P))
    with pytest.raises(RuntimeError, match="exceed the batch's capacity"):
        sd.reload_indexed(*X.ReadSet(rs.reads + rs.reads).args())
    sd.close()
    plain = hip.Seeder(P.k, P.w, P.max_occ, *small.plain_args(S.KNOWN_R))
    with pytest.raises(RuntimeError, match="call ba_seeding_reload"):
        plain.reload_indexed(*small.args())
    plain.run()
    assert plain.n_hits == sum(len(e["q_hit"]) for e in small.expected(S.KNOWN_R, P))
    plain.close()


def mapping():
    if not _mapping:
        ms = X.MappingSet()
        _mapping.update(ms=ms, exps=ms.reads.expected(ms.ref, X.MAP_PARAMS))
    return _mapping["ms"], _mapping["exps"]


def test_the_hand_off_from_an_indexed_seeder(hip):
    """AnchorChainer.from_seeder on the indexed seeder against a chainer built from the host copy of the hits: dp() and results()."""
    ms, exps = mapping()
    P, CP = X.MAP_PARAMS, X.MAP_CHAINING
    ix = hip.RefIndex(P.k, P.w, ms.ref)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *ms.reads.args())
    ix.close()
    sd.run()
    compare(sd, P.k, exps)
    first, q, r, ln, _ = sd.results()
    a = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()
    b = hip.AnchorChainer(*CP, first, q, r, ln)
    a.run(); b.run()
    for x, y in zip(a.dp(), b.dp()):
        assert np.array_equal(x, y)
    ra, rb = a.results(), b.results()
    assert ra.keys() == rb.keys()
    for key in ra:
        assert np.array_equal(ra[key], rb[key]), key
    a.close(); b.close()


def test_bytes_of_one_reference_and_many_reads_to_alignments(hip, oracle):
    """The whole path with candidate windows (margin 64): the chains equal the chaining model's, the windowed arguments the windows
    model's, the chain batch's results and runs the chain model's over the oracle on the windowed input, and the rank-0 chain of every read
    on its true strand, shifted back, overlaps the interval the read was drawn from."""
    ms, exps = mapping()
    P, CP = X.MAP_PARAMS, X.MAP_CHAINING
    rs, n = ms.reads, len(ms.reads)
    ix = hip.RefIndex(P.k, P.w, ms.ref)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *rs.args())
    sd.run()
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close(); ix.close()
    ch.run()
    res = ch.results()
    chains = X.model_chains(ms, exps)
    assert list(zip(res["chain_problem"].tolist(), res["chain_rank"].tolist())) == [(p, rank) for p, rank, _ in chains]
    cs, shift = X.windowed_chain_set(ms, chains)
    pool = np.concatenate([rs.pool, np.frombuffer(ms.ref + bytes(8), np.uint8)])   # the reference behind the reads
    r_off, r_len = np.full(n, len(rs.pool), np.uint64), np.full(n, len(ms.ref), np.uint32)
    plain = ch.chain_batch_args(pool, rs.q_off, rs.q_len, r_off, r_len, rs.strand)
    assert not hasattr(ch, "last_window_shift") and (plain[4] == len(ms.ref)).all()   # without a margin: as before
    args = ch.chain_batch_args(pool, rs.q_off, rs.q_len, r_off, r_len, rs.strand, margin=X.MAP_MARGIN)
    assert np.array_equal(ch.last_window_shift, shift)
    assert np.array_equal(args[3] - np.uint64(len(rs.pool)), shift) and np.array_equal(args[4], cs.r_len) and np.array_equal(args[7], cs.r_anchor)
    assert np.array_equal(args[6], cs.q_anchor) and np.array_equal(args[8], cs.anchor_len) and np.array_equal(args[9], cs.strand)
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, mode, *args)
    assert cb.n == len(chains)
    out, _ = check_chain_batch(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, mode, cs, cb=cb)
    at = {(p, rank): c for c, (p, rank, _) in enumerate(chains)}
    for i in range(len(ms.origin)):
        c = at[(ms.true_problem(i), 0)]
        assert X.overlaps_origin(ms, i, int(out["r_start"][c]) + int(shift[c]), int(out["r_end"][c]) + int(shift[c])), i
    cb.close(); ch.close()
