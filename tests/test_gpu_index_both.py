"""Both strands at once on the MI355X: a canonical RefIndex against entries(), Seeder.indexed_both against hits() -- all bit for bit
(tests/index_both_ref.py; tests/test_index_both_ref.py holds the cases against the rule's neighbouring mistakes) --, the tie to the
listed-twice path on the device, the life cycle and the refusals of mixed use, and the whole path from the bytes of four sequences and 24
reads, each listed once, to PAF lines."""
import numpy as np
import pytest

from tests import chaining_ref as C, index_both_ref as B, index_multi_ref as M, index_ref as X, seeding_ref as S, select_ref
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP, check as check_chain_batch
from tests.test_gpu_chaining import compare as compare_chains

pytestmark = pytest.mark.gpu

_mapping = {}   # the read set of the whole path and the models' results, built once


def check_index(ix, seqs, k, w, name):
    code, pos, longest = B.entries(seqs, k, w)
    c = ix.counts()
    assert ix.canonical and (c["k"], c["w"], c["ref_len"]) == (k, w, sum(len(s) for s in seqs)), name
    assert (c["n_entries"], c["longest_run"]) == (len(code), longest), name
    got_code, got_pos = ix.entries()
    assert np.array_equal(got_code, code) and np.array_equal(got_pos, pos), name   # pos: with the strand in bit 31
    assert ix.sequences().tolist() == M.seq_start(seqs), name


def compare(sd, k, exps):
    """Every read's sketch and every hit of every problem, none left out. exps: index_both_ref.expected()."""
    probs = B.per_problem(exps)
    assert sd.n_reads == len(exps) and sd.n == len(probs)
    assert sd.read.tolist() == [r for r in range(len(exps)) for _ in (0, 1)] and sd.strand.tolist() == [0, 1] * len(exps)
    sk = sd.sketch()
    first, q_hit, r_hit, hit_len, per = sd.results()
    assert per.tolist() == [len(p["q_hit"]) for p in probs]
    assert first.tolist() == np.concatenate([[0], np.cumsum([len(p["q_hit"]) for p in probs])]).tolist()
    assert len(q_hit) == len(r_hit) == len(hit_len) == int(first[-1]) and (hit_len == k).all()
    assert sk["q_first"].tolist() == np.concatenate([[0], np.cumsum([len(e["q_pos"]) for e in exps])]).tolist()
    assert sk["r_first"].tolist() == [0] * (sd.n_reads + 1) and len(sk["r_pos"]) == len(sk["r_code"]) == 0
    for r, e in enumerate(exps):
        a, b = int(sk["q_first"][r]), int(sk["q_first"][r + 1])
        assert np.array_equal(sk["q_pos"][a:b], e["q_pos"]) and np.array_equal(sk["q_code"][a:b], e["q_code"]), r
    for p, e in enumerate(probs):
        a, b = int(first[p]), int(first[p + 1])
        assert np.array_equal(q_hit[a:b], e["q_hit"]), p
        assert np.array_equal(r_hit[a:b], e["r_hit"]), p
    c = sd.counts()
    assert (c["n_hits"], c["n_q_seeds"], c["n_r_seeds"]) == (len(q_hit), len(sk["q_pos"]), 0)


def run(hip, seqs, rs, P):
    ix = hip.RefIndex.from_sequences(P.k, P.w, seqs, canonical=True)
    sd = hip.Seeder.indexed_both(ix, P.max_occ, P.max_ref_occ, *rs.args())
    ix.close()   # the seeder shares the index's buffers, and its sequence table
    sd.run()
    exps = B.expected(rs.reads, seqs, P)
    compare(sd, P.k, exps)
    assert sd.seq_start.tolist() == M.seq_start(seqs)
    t = sd.times()
    assert set(t) == {"sketch_ms", "sort_ms", "match_ms"} and all(v >= 0 for v in t.values())
    sd.close()
    return exps


# ------------------------------------------------------------------ the index sketch
@pytest.mark.parametrize("k, w", B.INDEX_KW)
def test_the_entries_of_a_canonical_index(hip, k, w):
    """entries(), with their strand bits, and longest_run: window counts around one and two spans, ACGT repeats (palindromes at k = 4),
    lower case and other bytes with a run of N across a seam, inverted repeats, and four sequences with a match across a junction."""
    for name, seqs in B.index_cases(k, w).items():
        ix = hip.RefIndex.from_sequences(k, w, seqs, canonical=True)
        check_index(ix, seqs, k, w, name)
        t = ix.times()
        assert set(t) == {"sketch_ms", "sort_ms", "table_ms"} and all(v >= 0 for v in t.values())
        ix.close()
        if len(seqs) == 1 and name.startswith("random"):
            ix = hip.RefIndex(k, w, seqs[0], canonical=True)   # the constructor's flag: the same index
            check_index(ix, seqs, k, w, name)
            ix.close()


# ------------------------------------------------------------------ the read sketch
@pytest.mark.parametrize("k, w", B.INDEX_KW)
def test_the_sketches_of_reads_at_the_chunk_edges(hip, k, w):
    """sketch() and every hit: reads of 0, k - 1 and k bytes, reads of 63, 64, 65 and 129 windows from either strand, lower case and
    other bytes, inverted repeats, palindromes."""
    seqs, rs = B.read_cases(k, w)
    run(hip, seqs, rs, B.Params(k, w, 8, 8))
    run(hip, seqs, rs, B.Params(k, w, B.NO_CAP, B.NO_CAP))


# ------------------------------------------------------------------ the lookup
def test_the_known_answers(hip):
    rs = B.Reads([S.KNOWN_Q, S.KNOWN_Q_MINUS, b"ACGNACGNNACG", b"", b"CCCCCCCCCCCCC"])
    exps = run(hip, [S.KNOWN_R], rs, B.Params(5, 4, 2, B.NO_CAP))
    assert list(zip(exps[0]["problems"][0]["q_hit"].tolist(), exps[0]["problems"][0]["r_hit"].tolist()))[:4] == [(3, 5), (29, 5), (4, 6), (30, 6)]
    exps = run(hip, [S.KNOWN_R], rs, B.Params(5, 3, 4, B.NO_CAP))
    assert list(zip(exps[1]["problems"][1]["q_hit"].tolist(), exps[1]["problems"][1]["r_hit"].tolist()))[:2] == [(11, 3), (13, 5)]
    run(hip, [S.KNOWN_R], rs, B.Params(5, 3, 4, 1))


def test_hits_on_both_strands_within_one_step(hip):
    """A read of more than 128 entries with plus and minus hits in every step of 64, a read with minus hits only, a read with none."""
    seqs, rs = B.strands_case()
    for caps in ((8, 8), (B.NO_CAP, B.NO_CAP)):
        exps = run(hip, seqs, rs, B.Params(11, 3, *caps))
        assert [len(p["q_hit"]) > 0 for p in B.per_problem(exps)] == [True, True, False, True, False, False]


@pytest.mark.parametrize("max_occ, max_ref_occ", B.OCC_CAPS)
def test_codes_at_and_over_either_cap_split_across_the_strands(hip, max_occ, max_ref_occ):
    for k in (13, 16):
        seqs, rs = B.occ_case(k, max_occ, max_ref_occ)
        exps = run(hip, seqs, rs, B.Params(k, 1, max_occ, max_ref_occ))
        assert sum(len(p["q_hit"]) for p in exps[0]["problems"]) == max_occ * max_ref_occ
        run(hip, seqs, rs, B.Params(k, 1, max_occ + 1, max_ref_occ + 1))


# ------------------------------------------------------------------ the hit sort
@pytest.mark.parametrize("extra", [0, 1])
def test_the_sort_of_a_minus_problems_hits_at_and_over_what_fits_in_lds(hip, extra):
    seqs, rs = B.hit_sort_case(extra)
    exps = run(hip, seqs, rs, B.Params(12, 1, 64, 128))
    assert [len(p["q_hit"]) for p in B.per_problem(exps)] == [0, 0, 1, 0, 0, X.SORT_LDS + extra, 2, 0]


# ------------------------------------------------------------------ the tie to the listed-twice path, on the device
@pytest.mark.parametrize("k", [5, 11, 15])
def test_odd_k_without_windows_and_caps_equals_the_reads_listed_twice(hip, k):
    seqs, rs = B.tie_case(k)
    both = hip.RefIndex.from_sequences(k, 1, seqs, canonical=True)
    plain = hip.RefIndex.from_sequences(k, 1, seqs)
    a = hip.Seeder.indexed_both(both, B.NO_CAP, B.NO_CAP, *rs.args())
    b = hip.Seeder.indexed(plain, B.NO_CAP, B.NO_CAP, *rs.listed_twice().args())
    a.run(); b.run()
    assert a.n == b.n == 2 * len(rs) and a.n_hits > 0
    for x, y in zip(a.results(), b.results()):   # hit_first, q_hit, r_hit, hit_len, hits_per_problem
        assert x.dtype == y.dtype and np.array_equal(x, y)
    a.close(); b.close(); both.close(); plain.close()


# ------------------------------------------------------------------ the life cycle and mixed use
def test_lifecycle(hip):
    P = B.Params(5, 4, 2, B.NO_CAP)
    rs = B.Reads([S.KNOWN_Q, S.KNOWN_Q_MINUS, b"ACGNACGNNACG", b"", b"CCCCCCCCCCCCC"])
    ix = hip.RefIndex(P.k, P.w, S.KNOWN_R, canonical=True)
    sd = hip.Seeder.indexed_both(ix, P.max_occ, P.max_ref_occ, *rs.args())
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    ix.close()   # the index before the seeder: the seeder shares its buffers
    sd.run()
    compare(sd, P.k, B.expected(rs.reads, [S.KNOWN_R], P))
    small = B.Reads(rs.reads[1:3])
    sd.reload_indexed_both(*small.args())
    assert (sd.n, sd.n_reads) == (4, 2)
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    sd.run()
    compare(sd, P.k, B.expected(small.reads, [S.KNOWN_R], P))
    sd.reload_indexed_both(*rs.args())   # back to the first set: its capacity
    sd.run()
    compare(sd, P.k, B.expected(rs.reads, [S.KNOWN_R], P))
    with pytest.raises(RuntimeError, match=r"reload: 10 reads exceed the batch's capacity of 5"):
        sd.reload_indexed_both(*B.Reads(rs.reads + rs.reads).args())
    n_problems, n_reads = hip.C.c_uint64(), hip.C.c_uint64()   # (the refused reload left the loaded reads as they were)
    assert hip.lib().ba_seeding_problems(sd._h, hip.C.byref(n_problems), hip.C.byref(n_reads)) == 0
    assert (n_problems.value, n_reads.value) == (10, 5)
    sd.close()


def test_mixed_use_is_refused(hip):
    rs = B.Reads([S.KNOWN_Q, S.KNOWN_Q_MINUS])
    twice = rs.listed_twice()
    both, plain = hip.RefIndex(5, 4, S.KNOWN_R, canonical=True), hip.RefIndex(5, 4, S.KNOWN_R)
    assert both.canonical and not plain.canonical
    flag = hip.C.c_int(7)
    for ix, want in ((both, 1), (plain, 0)):
        assert hip.lib().ba_ref_index_is_canonical(ix._h, hip.C.byref(flag)) == 0 and flag.value == want
    with pytest.raises(RuntimeError, match="ba_seeding_create_indexed: the index is canonical .* call ba_seeding_create_indexed_both"):
        hip.Seeder.indexed(both, 2, B.NO_CAP, *twice.args())
    with pytest.raises(RuntimeError, match="ba_seeding_create_indexed_both: the index is not canonical .* call ba_seeding_create_indexed$"):
        hip.Seeder.indexed_both(plain, 2, B.NO_CAP, *rs.args())
    sd = hip.Seeder.indexed_both(both, 2, B.NO_CAP, *rs.args())
    with pytest.raises(RuntimeError, match="ba_seeding_reload: .* call ba_seeding_reload_indexed_both"):
        sd.reload(*twice.plain_args(S.KNOWN_R))
    with pytest.raises(RuntimeError, match="ba_seeding_reload_indexed: .* call ba_seeding_reload_indexed_both"):
        sd.reload_indexed(*twice.args())
    sd.run()   # the refusals left it as it was
    compare(sd, 5, B.expected(rs.reads, [S.KNOWN_R], B.Params(5, 4, 2, B.NO_CAP)))
    sd.close()
    one = hip.Seeder.indexed(plain, 2, B.NO_CAP, *twice.args())
    with pytest.raises(RuntimeError, match="ba_seeding_reload_indexed_both: .* call ba_seeding_reload_indexed$"):
        one.reload_indexed_both(*rs.args())
    one.close()
    pair = hip.Seeder(5, 4, 2, *twice.plain_args(S.KNOWN_R))
    with pytest.raises(RuntimeError, match="ba_seeding_reload_indexed_both: .* call ba_seeding_reload$"):
        pair.reload_indexed_both(*rs.args())
    pair.close(); both.close(); plain.close()


def test_more_than_2_28_hits_are_refused_with_the_read_and_the_strand(hip):
    """seeding_ref.over_limit_set's 17 000-base homopolymer, as poly-T against a poly-A canonical index at w 1 without caps: the canonical code
    is poly-A's on either side, with the read's entries on strand 1, so the minus problem of read 1 has 16 986 x 16 986 hits. The count
    pass sees it, nothing is emitted, and the seeder stays usable."""
    k, n = 15, 17000
    rs = B.Reads([b"ACGTACGTACGTACGTACGT", b"T" * n, b"ACGTTGCATGGACCTAGGATCCAGT"])
    ix = hip.RefIndex(k, 1, b"A" * n, canonical=True)
    assert ix.counts()["longest_run"] == n - k + 1
    sd = hip.Seeder.indexed_both(ix, B.NO_CAP, B.NO_CAP, *rs.args())
    ix.close()
    each = (n - k + 1) ** 2
    assert each > 1 << 28
    with pytest.raises(RuntimeError, match=rf"more than 2\^28 hits: read 1 on strand 1 alone has {each}, with {1 << 28} left after the problems before it"):
        sd.run()
    with pytest.raises(RuntimeError, match="ba_seeding_run has not been called"):
        sd.results()
    sd.reload_indexed_both(*B.Reads([b"T" * 40, b"A" * 30]).args())   # 26 x 16 986 minus hits, then 16 x 16 986 plus hits
    sd.run()
    assert sd.counts()["hits_per_problem"].tolist() == [0, 26 * (n - k + 1), 16 * (n - k + 1), 0]
    sd.close()


# ------------------------------------------------------------------ the hand-off and the whole path
def mapping():
    if not _mapping:
        ms = B.BothMappingSet()
        exps = ms.expected_hits()
        _mapping.update(ms=ms, exps=exps, chains=M.model_chains(exps, ms.start, X.MAP_CHAINING, B.MAP_PARAMS.k))
    return _mapping["ms"], _mapping["exps"], _mapping["chains"]


def test_the_hand_off_from_a_both_strand_seeder(hip):
    """AnchorChainer.from_seeder sees 2 n problems and is bounded by the index's sequences: dp() and results() equal the bounded model on
    the model's hits."""
    ms, exps, _ = mapping()
    P, CP = B.MAP_PARAMS, X.MAP_CHAINING
    ix = hip.RefIndex.from_sequences(P.k, P.w, ms.pool, ms.seq_off, ms.seq_len, canonical=True)
    sd = hip.Seeder.indexed_both(ix, P.max_occ, P.max_ref_occ, ms.pool, ms.once.q_off, ms.once.q_len)
    ix.close()
    sd.run()
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close()
    assert ch.n == 2 * B.MAP_READS and ch.seq_start.tolist() == ms.start
    ch.run()
    ps = C.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exps])
    compare_chains(ch, ps, [M.chain_bounded(CP, q, r, L, ms.start) for q, r, L in ps.problems])
    ch.close()


def test_bytes_of_four_sequences_and_reads_listed_once_to_paf_lines(hip, oracle):
    ms, exps, chains = mapping()
    P, CP = B.MAP_PARAMS, X.MAP_CHAINING
    once, n_reads = ms.once, B.MAP_READS
    ix = hip.RefIndex.from_sequences(P.k, P.w, ms.pool, ms.seq_off, ms.seq_len, canonical=True)
    sd = hip.Seeder.indexed_both(ix, P.max_occ, P.max_ref_occ, ms.pool, once.q_off, once.q_len)
    sd.run()
    compare(sd, P.k, B.expected(once.reads, ms.seqs, P))
    q_off, q_len, strand, read_of_problem = once.q_off[sd.read], once.q_len[sd.read], sd.strand, sd.read
    ch = hip.AnchorChainer.from_seeder(*CP, sd)
    sd.close(); ix.close()
    ch.run()
    res = ch.results()
    assert list(zip(res["chain_problem"].tolist(), res["chain_rank"].tolist())) == [(p, rank) for p, rank, _ in chains]
    cs, seq, shift = M.windowed_chain_set(ms, chains)
    args = ch.chain_batch_args(ms.pool, q_off, q_len, None, None, strand, margin=X.MAP_MARGIN, seq_off=ms.seq_off, seq_len=ms.seq_len)
    assert np.array_equal(ch.last_window_shift, shift) and np.array_equal(ch.last_window_seq, seq)
    assert np.array_equal(args[4], cs.r_len) and np.array_equal(args[7], cs.r_anchor) and np.array_equal(args[6], cs.q_anchor)
    assert np.array_equal(args[8], cs.anchor_len) and np.array_equal(args[9], cs.strand)
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    cb = hip.ChainBatchAligner(NUC, DNA_GAPS, (32, 256), X_DROP, mode, *args)
    assert cb.n == len(chains)
    out, _ = check_chain_batch(hip, oracle, NUC, DNA_GAPS, (32, 256), X_DROP, mode, cs, cb=cb)   # the alignments of the model's chains
    rep = cb.report()
    stats, cigars = rep.stats(), rep.text_list()
    cp = res["chain_problem"]
    paf = hip.paf_columns(out, stats, q_len[cp], strand[cp], ch.last_window_shift)
    read_of_chain = read_of_problem[cp].astype(np.uint32)
    support = np.diff(res["anchor_first"].astype(np.int64)).astype(np.uint32)
    sel = hip.Selector.from_chain_batch(*select_ref.GPU_PARAMS, cb, read_of_chain, support, n_reads)
    sel.run()
    picked = sel.results()
    names = [f"read_{i}" for i in range(n_reads)]
    lines = hip.paf_lines(names, once.q_len, B.MAP_NAMES, B.MAP_LENGTHS, paf, picked, cigars, target=ch.last_window_seq)
    # the lines built from the model's chains: their alignments (checked against the oracle above), the selection model over them
    model_sel = select_ref.select(select_ref.GPU_PARAMS, read_of_chain, out["score"], out["q_start"], out["q_end"], q_len[cp], strand[cp], support,
                                  np.asarray(out["status"]) != 0, n_reads)
    model_sel = {key: np.asarray(v) for key, v in model_sel.items()}
    assert lines == hip.paf_lines(names, once.q_len, B.MAP_NAMES, B.MAP_LENGTHS, paf, model_sel, cigars, target=seq)
    kept = picked["kept"].tolist()
    assert len(lines) == len(kept) >= n_reads
    for i, (s, lo, hi, st) in enumerate(ms.origin):   # every plain read's primary: its true sequence and strand, over its true interval
        prim = [c for c in kept if int(read_of_chain[c]) == i and int(picked["cls"][c]) == hip.SEL_PRIMARY]
        assert len(prim) == 1, i
        c = prim[0]
        assert int(seq[c]) == s and int(strand[cp[c]]) == st and int(paf["t_start"][c]) < hi and lo < int(paf["t_end"][c]), i
        assert int(paf["t_start"][c]) >= lo - 30 and int(paf["t_end"][c]) <= hi + 30 and int(paf["t_end"][c]) - int(paf["t_start"][c]) > (hi - lo) // 2, i
        line = [x for x in lines if x.startswith(f"read_{i}\t") and "tp:A:P" in x][0].split("\t")
        assert (line[4], line[5]) == ("+-"[st], B.MAP_NAMES[s])
    chim = {B.MAP_NAMES[int(seq[c])] for c in kept if int(read_of_chain[c]) == ms.chimeric and int(picked["cls"][c]) != hip.SEL_SECONDARY}
    assert chim == {"contig_b", "chr_d"}   # a primary and a supplementary line
    sel.close(); cb.close(); ch.close()
