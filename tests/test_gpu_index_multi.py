"""Several sequences in one index on the MI355X: RefIndex.from_sequences against entries_multi, an indexed Seeder over it against
hits_multi, the bounded AnchorChainer against fill_bounded / chain_bounded -- all bit for bit (tests/index_multi_ref.py) --, and the whole
path from the bytes of four sequences and twelve reads to PAF lines that name the right sequence in its own coordinates."""
import numpy as np
import pytest

from tests import chaining_ref as C, index_multi_ref as M, index_ref as X, seeding_ref as S, select_ref
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP, check as check_chain_batch
from tests.test_gpu_chaining import compare as compare_chains
from tests.test_gpu_index import compare as compare_hits

pytestmark = pytest.mark.gpu

_mapping = {}   # the read set of the whole path and the models' results, built once


def check_index(ix, seqs, k, w, name):
    code, pos, longest = M.entries_multi(seqs, k, w)
    c = ix.counts()
    assert (c["k"], c["w"], c["ref_len"]) == (k, w, sum(len(s) for s in seqs)), name
    assert (c["n_entries"], c["longest_run"]) == (len(code), longest), name
    got_code, got_pos = ix.entries()
    assert np.array_equal(got_code, code) and np.array_equal(got_pos, pos), name
    assert ix.sequences().tolist() == M.seq_start(seqs), name


@pytest.mark.parametrize("k, w", X.SEAM_KW)
def test_entries_of_several_sequences(hip, k, w):
    """entries() and counts() against the union of every sequence's own sketch: junctions at SPAN - 1, SPAN and SPAN + 1 windows of the
    sequence before, short sequences between long ones, poly-A on both sides of a junction, 2000 short sequences."""
    sets = M.seam_sets(k, w)
    for name, seqs in sets.items():
        ix = hip.RefIndex.from_sequences(k, w, seqs)
        check_index(ix, seqs, k, w, name)
        t = ix.times()
        assert set(t) == {"sketch_ms", "sort_ms", "table_ms"} and all(v >= 0 for v in t.values())
        ix.close()
    a, b = sets["poly_a_across_the_junction"]
    joined = X.entries(a + b, k, w)[1]
    assert ((joined > len(a) - k) & (joined < len(a))).any()   # the case is what it says: the concatenation selects one across it


@pytest.mark.parametrize("k, w", X.SEAM_KW)
def test_one_sequence_equals_the_single_reference_index(hip, k, w):
    for name in ("random_%d" % (X.SPAN + 1), "n_run", "all_t", "one_window", "shorter_than_k", "empty"):
        ref = X.seam_references(k, w)[name]
        a, b = hip.RefIndex.from_sequences(k, w, [ref]), hip.RefIndex(k, w, ref)
        assert a.counts() == b.counts(), name
        for x, y in zip(a.entries(), b.entries()):
            assert np.array_equal(x, y), name
        assert a.sequences().tolist() == b.sequences().tolist() == [0, len(ref)]
        rs = X.ReadSet([(ref[:300], 0), (S.oriented(ref[100:500], 1), 1)])
        if name.startswith("random"):   # the table-dependent counts: hits through either index, with a cap on the reference's codes
            sa, sb = hip.Seeder.indexed(a, 4, 2, *rs.args()), hip.Seeder.indexed(b, 4, 2, *rs.args())
            sa.run(); sb.run()
            for x, y in zip(sa.results(), sb.results()):
                assert np.array_equal(x, y)
            assert sa.n_hits > 0 and sa.seq_start.tolist() == [0, len(ref)] and sb.seq_start is None
            sa.close(); sb.close()
        a.close(); b.close()


def test_sequences_anywhere_in_the_pool(hip):
    """Only seq_off says where a sequence lies: apart from one another, out of order, one of them used twice."""
    rng = np.random.default_rng(77)
    parts = [S.dna(rng, n) for n in (900, 40, 1500)]
    pool = np.frombuffer(b"###" + parts[2] + b"#" + parts[0] + b"##" + parts[1], np.uint8)
    off = [3 + 1500 + 1, 3 + 1500 + 1 + 900 + 2, 0, 3, 3 + 1500 + 1]
    seqs = [parts[0], parts[1], b"", parts[2], parts[0]]
    ix = hip.RefIndex.from_sequences(11, 5, pool, off, [len(s) for s in seqs])
    check_index(ix, seqs, 11, 5, "apart")
    ix.close()


def run_hits(hip, seqs, rs, P):
    ix = hip.RefIndex.from_sequences(P.k, P.w, seqs)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *rs.args())
    ix.close()   # the seeder shares the index's buffers, and its sequence table
    sd.run()
    exps = [M.hits_multi(q, seqs, P, s) for q, s in rs.reads]
    compare_hits(sd, P.k, exps)
    assert sd.seq_start.tolist() == M.seq_start(seqs)
    sd.close()
    return exps


def test_hits_against_three_sequences_and_an_empty_one(hip):
    seqs = [S.KNOWN_R, b"", S.KNOWN_R[10:] + S.KNOWN_R[:10], S.oriented(S.KNOWN_R, 1)]
    rs = X.known_reads()
    for k, w, occ, ref_occ in ((5, 4, 2, X.NO_CAP), (5, 4, 1, X.NO_CAP), (5, 3, 4, X.NO_CAP), (5, 4, 2, 2), (5, 4, 2, 1)):
        exps = run_hits(hip, seqs, rs, X.Params(k, w, occ, ref_occ))
        assert [len(e["q_hit"]) for e in exps[4:]] == [0, 0, 0]   # no valid k-mer, empty, no hit
    start = M.seq_start(seqs)
    e = M.hits_multi(S.KNOWN_Q, seqs, X.Params(5, 4, 2, X.NO_CAP))
    assert all(sum(1 for a in e["r_hit"].tolist() if lo <= a < hi) > 0 for lo, hi in zip(start, start[1:]) if hi > lo)   # hits in every sequence


@pytest.mark.parametrize("max_occ, max_ref_occ", [(1, 1), (2, 3), (64, 2)])
def test_a_cap_that_only_the_sum_over_two_sequences_exceeds(hip, max_occ, max_ref_occ):
    for k in (13, 16):
        seqs, rs = M.cap_sum_case(k, max_occ, max_ref_occ)
        exps = run_hits(hip, seqs, rs, X.Params(k, 1, max_occ, max_ref_occ))
        assert len(exps[0]["q_hit"]) == max_ref_occ * max_occ   # the k-mer exactly at the cap stays, the one over it in the sum goes
        over = run_hits(hip, seqs, rs, X.Params(k, 1, max_occ, max_ref_occ + 1))
        assert len(over[0]["q_hit"]) == (2 * max_ref_occ + 1) * max_occ


# ------------------------------------------------------------------ the bounded fill
@pytest.fixture(scope="module")
def bounded():
    return M.bounded_sets()


@pytest.mark.parametrize("name", ["junction", "random", "inside_a_chunk", "at_the_ring_wrap"])
def test_the_bounded_fill_and_its_chains(hip, bounded, name):
    """dp() and results() of a chainer with a sequence table against fill_bounded / chain_bounded; the same problems without a table still
    equal chaining_ref."""
    P, ps, start = bounded[name]
    want = [M.chain_bounded(P, q, r, L, start) for q, r, L in ps.problems]
    plain = ps.expected(P)
    assert any(a["f"] != b["f"] for a, b in zip(want, plain))   # a chainer that ignored the table would fail
    ch = hip.AnchorChainer(*P, *ps.args(), seq_start=start)
    assert ch.seq_start.tolist() == start
    ch.run()
    compare_chains(ch, ps, want)
    ch.reload(*ps.args())   # the table stays
    ch.run()
    compare_chains(ch, ps, want)
    ch.close()
    ch = hip.AnchorChainer(*P, *ps.args())
    assert ch.seq_start is None
    ch.run()
    compare_chains(ch, ps, plain)
    ch.close()


def test_the_junction_problem_gives_two_chains(hip, bounded):
    P, ps, start = bounded["junction"]
    ch = hip.AnchorChainer(*P, *ps.args(), seq_start=start)
    ch.run()
    res = ch.results()
    assert res["chains_per_problem"].tolist() == [2]
    ends = [(int(res["r_anchor"][int(a)]), int(res["r_anchor"][int(b) - 1] + res["anchor_len"][int(b) - 1]))
            for a, b in zip(res["anchor_first"][:-1], res["anchor_first"][1:])]
    assert sorted(ends)[0][1] <= 1000 <= sorted(ends)[1][0]
    with pytest.raises(RuntimeError, match=r"problem 0, anchor 4: .* leaves its sequence, which ends at 970"):
        hip.AnchorChainer(*P, *ps.args(), seq_start=[0, 970, 3000])
    ch.close()


def test_one_sequence_bounded_equals_unbounded(hip):
    P, ps = C.gpu_sets()["sizes"]
    a, b = hip.AnchorChainer(*P, *ps.args(), seq_start=[0, 1 << 30]), hip.AnchorChainer(*P, *ps.args())
    a.run(); b.run()
    for x, y in zip(a.dp(), b.dp()):
        assert np.array_equal(x, y)
    ra, rb = a.results(), b.results()
    for key in rb:
        assert np.array_equal(ra[key], rb[key]), key
    a.close(); b.close()


# ------------------------------------------------------------------ the whole path
def mapping():
    if not _mapping:
        ms = M.MultiMappingSet()
        exps = ms.expected_hits()
        _mapping.update(ms=ms, exps=exps, chains=M.model_chains(exps, ms.start))
    return _mapping["ms"], _mapping["exps"], _mapping["chains"]


def test_the_hand_off_from_a_seeder_over_several_sequences(hip):
    """AnchorChainer.from_seeder on a seeder of a multi-sequence index is bounded without being asked: dp() and results() equal the bounded
    model on the seeder's hits, and differ from the plain rule's on the chimeric read."""
    ms, exps, _ = mapping()
    P, CP = X.MAP_PARAMS, X.MAP_CHAINING
    ix = hip.RefIndex.from_sequences(P.k, P.w, ms.pool, ms.seq_off, ms.seq_len)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *ms.reads.args())
    ix.close()
    sd.run()
    compare_hits(sd, P.k, exps)
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()
    assert ch.seq_start.tolist() == ms.start
    ch.run()
    ps = C.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exps])
    want = [M.chain_bounded(CP, q, r, L, ms.start) for q, r, L in ps.problems]
    compare_chains(ch, ps, want)
    assert want[2 * ms.chimeric]["f"] != ps.expected(CP)[2 * ms.chimeric]["f"]
    ch.close()


def test_bytes_of_several_sequences_and_many_reads_to_paf_lines(hip, oracle):
    ms, exps, chains = mapping()
    P, CP = X.MAP_PARAMS, X.MAP_CHAINING
    rs, n_reads = ms.reads, len(ms.reads) // 2
    ix = hip.RefIndex.from_sequences(P.k, P.w, ms.pool, ms.seq_off, ms.seq_len)
    sd = hip.Seeder.indexed(ix, P.max_occ, P.max_ref_occ, *rs.args())
    sd.run()
    compare_hits(sd, P.k, exps)
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()
    ch.run()
    res = ch.results()
    assert list(zip(res["chain_problem"].tolist(), res["chain_rank"].tolist())) == [(p, rank) for p, rank, _ in chains]
    cs, seq, shift = M.windowed_chain_set(ms, chains)
    with pytest.raises(ValueError, match="r_off and r_len must be None and a margin is required"):
        ch.chain_batch_args(ms.pool, rs.q_off, rs.q_len, None, None, rs.strand, seq_off=ms.seq_off, seq_len=ms.seq_len)
    args = ch.chain_batch_args(ms.pool, rs.q_off, rs.q_len, None, None, rs.strand, margin=X.MAP_MARGIN, seq_off=ms.seq_off, seq_len=ms.seq_len)
    assert np.array_equal(ch.last_window_shift, shift) and np.array_equal(ch.last_window_seq, seq)
    assert np.array_equal(args[4], cs.r_len) and np.array_equal(args[7], cs.r_anchor) and np.array_equal(args[6], cs.q_anchor)
    assert np.array_equal(args[8], cs.anchor_len) and np.array_equal(args[9], cs.strand)
    for c in range(len(chains)):   # every window lies inside its sequence, wherever that lies in the pool
        s = int(seq[c])
        assert int(shift[c]) + int(args[4][c]) <= M.MAP_LENGTHS[s] and int(args[3][c]) == int(ms.seq_off[s]) + int(shift[c]), c
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, mode, *args)
    assert cb.n == len(chains)
    out, _ = check_chain_batch(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, mode, cs, cb=cb)
    rep = cb.report()
    stats, cigars = rep.stats(), rep.text_list()
    cp = res["chain_problem"]
    paf = hip.paf_columns(out, stats, rs.q_len[cp], rs.strand[cp], ch.last_window_shift)
    # no located alignment crosses, and each is where paf_columns says, in its sequence's own coordinates
    g_start = np.array([ms.start[int(s)] for s in seq]) + paf["t_start"]
    g_end = np.array([ms.start[int(s)] for s in seq]) + paf["t_end"]
    loc = ix.locate(g_start, g_end)
    assert np.array_equal(loc["seq"], seq) and not loc["crosses"].any()
    assert np.array_equal(loc["local_start"], paf["t_start"]) and np.array_equal(loc["local_end"], paf["t_end"])
    ix.close()
    at = {(p, rank): c for c, (p, rank, _) in enumerate(chains)}
    for i, (s, lo, hi, _) in enumerate(ms.origin):   # every plain read's rank-0 chain on its true strand: the right sequence, over its origin
        c = at[(ms.true_problem(i), 0)]
        assert int(seq[c]) == s and int(paf["t_start"][c]) < hi and lo < int(paf["t_end"][c]), i
    two = [at[(2 * ms.chimeric, rank)] for rank in (0, 1)]
    assert sorted(int(seq[c]) for c in two) == [1, 3]   # the chimeric read: one chain on each of the two sequences
    read_of_chain = (cp // 2).astype(np.uint32)
    support = np.diff(res["anchor_first"].astype(np.int64)).astype(np.uint32)
    sel = hip.Selector.from_chain_batch(*select_ref.GPU_PARAMS, cb, read_of_chain, support, n_reads)
    sel.run()
    picked = sel.results()
    names = [f"read_{i}" for i in range(n_reads)]
    lines = hip.paf_lines(names, rs.q_len[0::2], M.MAP_NAMES, M.MAP_LENGTHS, paf, picked, cigars, target=ch.last_window_seq)
    kept = picked["kept"].tolist()
    assert len(lines) == len(kept) >= n_reads
    for line, c in zip(lines, kept):
        f = line.split("\t")
        s = int(seq[c])
        assert f[0] == names[int(read_of_chain[c])] and (f[5], int(f[6])) == (M.MAP_NAMES[s], M.MAP_LENGTHS[s]), line
        assert 0 <= int(f[7]) < int(f[8]) <= M.MAP_LENGTHS[s], line
        cg = cigars[c].decode() if isinstance(cigars[c], bytes) else cigars[c]
        assert f[4] == "+-"[int(rs.strand[cp[c]])] and f[-1] == "cg:Z:" + cg
    for i, (s, lo, hi, strand) in enumerate(ms.origin):   # every plain read's primary: its origin, by name
        prim = [c for c in kept if int(read_of_chain[c]) == i and int(picked["cls"][c]) == hip.SEL_PRIMARY]
        assert len(prim) == 1 and int(seq[prim[0]]) == s and int(rs.strand[cp[prim[0]]]) == strand, i
    chim = {M.MAP_NAMES[int(seq[c])] for c in kept if int(read_of_chain[c]) == ms.chimeric and int(picked["cls"][c]) != hip.SEL_SECONDARY}
    assert chim == {"contig_b", "chr_d"}   # a primary and a supplementary line
    sel.close(); cb.close(); ch.close()
