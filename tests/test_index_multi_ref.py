"""The models of tests/index_multi_ref.py against the models they extend and against exhaustive search, the junction problem that gives the
bounded fill its teeth, the read set of the whole path through the models alone, and paf_lines with a target per chain. No GPU."""
import numpy as np
import pytest

from tests import chaining_ref as C, index_multi_ref as M, index_ref as X, seeding_ref as S


def test_with_one_sequence_every_model_equals_the_one_it_extends():
    rng = np.random.default_rng(3)
    ref = S.dna(rng, 3000)
    for k, w in ((4, 1), (11, 5), (16, 64)):
        for a, b in zip(M.entries_multi([ref], k, w), X.entries(ref, k, w)):
            assert np.array_equal(a, b)
        P = X.Params(k, w, 3, 2)
        for read, s in ((S.mutate(rng, ref[500:900], 0.04), 0), (S.oriented(ref[100:500], 1), 1), (b"", 0)):
            got, want = M.hits_multi(read, [ref], P, s), X.hits(read, ref, P, s)
            assert got.keys() == want.keys()
            for key in want:
                assert np.array_equal(got[key], want[key]), key
    for name, (P, ps) in C.gpu_sets().items():
        if name in ("big", "tiny"):
            continue
        for q, r, L in ps.problems:
            want = C.chain(P, q, r, L)
            got = M.chain_bounded(P, q, r, L, [0, 1 << 30])
            assert got == want, name
    rng = np.random.default_rng(4)
    q_len, first, qa, ra, ln = [300, 200], [0, 2, 3], [10, 100, 50], [4000, 4100, 20], [8, 8, 8]
    for margin in (0, 64, 100000):
        r_off, r_len, r_anchor, seq, shift = M.chain_windows_seqs(q_len, first, qa, ra, ln, margin, [700], [5000])
        want = X.chain_windows(q_len, [700, 700], [5000, 5000], first, qa, ra, ln, margin)
        assert np.array_equal(r_off, want[0]) and np.array_equal(r_len, want[1]) and np.array_equal(r_anchor, want[2])
        assert np.array_equal(shift, want[3]) and seq.tolist() == [0, 0]
    loc = M.locate([5000], [0, 10, 5000], [0, 5000, 5000])
    assert loc["seq"].tolist() == [0, 0, 0] and loc["local_start"].tolist() == [0, 10, 5000] and loc["crosses"].tolist() == [0, 0, 0]


def test_entries_of_two_sequences_by_hand():
    """Two copies of one sequence: every entry twice, the second time 36 further on, and no entry of a k-mer across the junction."""
    k, w = 5, 4
    code, pos, longest = M.entries_multi([S.KNOWN_R, S.KNOWN_R], k, w)
    one = S.KNOWN_R_SKETCH
    assert sorted(pos.tolist()) == one + [p + len(S.KNOWN_R) for p in one]
    assert longest == 2 * X.entries(S.KNOWN_R, k, w)[2]
    joined = X.entries(S.KNOWN_R + S.KNOWN_R, k, w)[1].tolist()
    assert any(len(S.KNOWN_R) - k < p < len(S.KNOWN_R) for p in joined)   # (the concatenation does select one across it)
    assert not any(len(S.KNOWN_R) - k < p < len(S.KNOWN_R) for p in pos.tolist())


def test_the_reference_cap_counts_over_all_sequences_together():
    for max_occ, max_ref_occ in ((1, 1), (2, 3)):
        seqs, rs = M.cap_sum_case(13, max_occ, max_ref_occ)
        P = X.Params(13, 1, max_occ, max_ref_occ)
        q = rs.reads[0][0]
        per_seq = [len(X.hits(q, x, P)["q_hit"]) for x in seqs]
        got = M.hits_multi(q, seqs, P)
        # each sequence alone: both k-mers under the cap, (max_ref_occ + 1) + max_ref_occ entries with max_occ hits each; together: one over it
        assert sum(per_seq) == (2 * max_ref_occ + 1) * max_occ and len(got["q_hit"]) == max_ref_occ * max_occ
        assert len(M.hits_multi(q, seqs, P._replace(max_ref_occ=max_ref_occ + 1))["q_hit"]) == sum(per_seq)
        start = M.seq_start(seqs)
        assert all(not (a < start[2] < a + 13) for a in got["r_hit"].tolist())
        assert list(zip(got["r_hit"].tolist(), got["q_hit"].tolist())) == sorted(zip(got["r_hit"].tolist(), got["q_hit"].tolist()))


def test_the_bounded_fill_finds_the_best_chain_inside_one_sequence():
    rng = np.random.default_rng(13)
    differ = 0
    for k in range(150):
        n = int(rng.integers(1, 11))
        q, r, L = C.random_problem(rng, n, span=80, noise=0.4)
        cuts = sorted(set(int(x) for x in rng.integers(1, 90, int(rng.integers(1, 4)))))
        start = [0] + cuts + [cuts[-1], 200]
        ps = C.ProblemSet([M.drop_straddlers(q, r, L, start)])
        q, r, L = ps.problems[0]
        if not len(q):
            continue
        P = C.Params(int(rng.integers(1, 6)), int(rng.integers(0, 4)), 0, len(q), 1 << 30, 1 << 30, 1, -(1 << 30), 1)
        f, pred, _ = M.fill_bounded(P, q, r, L, start)
        assert max(f) == M.exhaustive_best_bounded(P, q, r, L, start), (k, q, r, L, start)
        assert all(p == C.NONE or M.seq_of(start, int(r[p])) == M.seq_of(start, int(r[i])) for i, p in enumerate(pred))
        differ += f != C.fill(P, q, r, L)[0]
    assert differ > 20   # the junctions matter in these problems


def test_the_junction_problem_has_teeth():
    """Colinear anchors across a junction, within max_dist and bandwidth: the plain rule links across it, the bounded one does not."""
    P, start = M.JUNCTION_PARAMS, M.JUNCTION_START
    q, r, L = M.junction_problem()
    assert M.drop_straddlers(q, r, L, start) == (q, r, L)
    assert any(a + n <= 1000 for a, n in zip(r, L)) and any(a >= 1000 for a in r)
    plain = C.chain(P, q, r, L)["chains"]
    assert len(plain) == 1 and len(plain[0][1]) == len(q)
    assert plain[0][1][0][1] < 1000 < plain[0][1][-1][1]
    bounded = M.chain_bounded(P, q, r, L, start)["chains"]
    assert len(bounded) == 2
    sides = sorted((min(a[1] for a in ch), max(a[1] + a[2] for a in ch)) for _, ch in bounded)
    assert sides[0][1] <= 1000 <= sides[1][0]
    assert sum(len(ch) for _, ch in bounded) == len(q)


def test_the_problem_sets_of_the_bounded_fill_are_what_they_say():
    sets = M.bounded_sets()
    for name, (P, ps, start) in sets.items():
        assert start[0] == 0 and all(a <= b for a, b in zip(start, start[1:])), name
        changed = 0
        for q, r, L in ps.problems:
            assert M.drop_straddlers(q.tolist(), r.tolist(), L.tolist(), start)[0] == q.tolist(), name
            changed += M.fill_bounded(P, q, r, L, start)[0] != C.fill(P, q, r, L)[0]
        assert changed, name   # a chainer that ignored the table would fail on every set
    P, ps, start = sets["inside_a_chunk"]
    q, r, L = ps.problems[0]
    at = r.tolist().index(start[1])
    assert len(q) > 64 and at % 64 not in (0, 63) and at > 64
    P, ps, start = sets["at_the_ring_wrap"]
    assert ps.problems[0][1].tolist().index(start[1]) == 128   # a ring of 128 slots for a look-back of 64: slot 0 again


def test_windows_and_locate_by_hand():
    seq_len, seq_off = [1000, 0, 500], [7000, 0, 100]
    #          a chain at the first base of sequence 0, one at its last base, one in sequence 2 under a margin larger than the sequence
    q_len = [100, 100, 100]
    first, qa, ra, ln = [0, 1, 2, 4], [0, 90, 10, 40], [0, 990, 1010, 1040], [10, 10, 10, 10]
    r_off, r_len, r_anchor, seq, shift = M.chain_windows_seqs(q_len, first, qa, ra, ln, 5, seq_off, seq_len)
    assert seq.tolist() == [0, 0, 2] and shift.tolist() == [0, 895, 0]
    assert r_off.tolist() == [7000, 7895, 100] and r_len.tolist() == [105, 105, 105] and r_anchor.tolist() == [0, 95, 10, 40]
    r_off, r_len, r_anchor, seq, shift = M.chain_windows_seqs(q_len, first, qa, ra, ln, 100000, seq_off, seq_len)
    assert shift.tolist() == [0, 0, 0] and r_len.tolist() == [1000, 1000, 500] and r_anchor.tolist() == [0, 990, 10, 40]
    with pytest.raises(ValueError, match="chain 0: anchor 0 ends outside"):
        M.chain_windows_seqs([100], [0, 1], [0], [995], [10], 5, seq_off, seq_len)   # over the junction at 1000
    loc = M.locate(seq_len, [0, 990, 990, 1000, 1500, 1499], [10, 1000, 1001, 1000, 1500, 1500])
    assert loc["seq"].tolist() == [0, 0, 0, 2, 2, 2]
    assert loc["local_start"].tolist() == [0, 990, 990, 0, 500, 499] and loc["local_end"].tolist() == [10, 1000, 1001, 0, 500, 500]
    assert loc["crosses"].tolist() == [0, 0, 1, 0, 0, 0]
    for a, b in ((5, 4), (0, 1501), (1501, 1501)):
        with pytest.raises(ValueError, match="interval 0"):
            M.locate(seq_len, [a], [b])


_mapping = {}


def mapping():
    if not _mapping:
        ms = M.MultiMappingSet()
        exps = ms.expected_hits()
        _mapping.update(ms=ms, exps=exps, chains=M.model_chains(exps, ms.start))
    return _mapping["ms"], _mapping["exps"], _mapping["chains"]


def test_the_model_pipeline_places_every_read_of_the_whole_path():
    """What tests/test_gpu_index_multi.py asserts of the device's results holds for the models: the GPU test cannot fail for its inputs'
    sake."""
    ms, exps, chains = mapping()
    assert [len(s) for s in ms.seqs] == list(M.MAP_LENGTHS) and len(ms.reads) == 24
    assert ms.origin[0][:3] == (0, 3400, 4000) and ms.origin[1][:3] == (3, 0, 600)
    at = {(p, rank): a for p, rank, a in chains}
    span = lambda a: (a[0][1], a[-1][1] + a[-1][2])   # noqa: E731
    for i, (s, lo, hi, _) in enumerate(ms.origin):
        a, b = span(at[(ms.true_problem(i), 0)])
        loc = M.locate(ms.seq_len, [a], [b])
        assert int(loc["seq"][0]) == s and not loc["crosses"][0], i
        assert int(loc["local_start"][0]) < hi and lo < int(loc["local_end"][0]), i
        assert len(at[(ms.true_problem(i), 0)]) >= 20, i
    c = 2 * ms.chimeric
    two = [span(at[(c, rank)]) for rank in (0, 1)]
    loc = M.locate(ms.seq_len, [x[0] for x in two], [x[1] for x in two])
    assert sorted(loc["seq"].tolist()) == [1, 3] and not loc["crosses"].any()
    # ... and the unbounded rule would have made one chain of the two
    e = exps[c]
    plain = C.chain(X.MAP_CHAINING, e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), X.MAP_PARAMS.k))["chains"]
    assert plain[0][1][0][1] < ms.start[2] < plain[0][1][-1][1]
    # every chain's window lies inside its sequence
    flat = [x for _, _, a in chains for x in a]
    first = np.concatenate([[0], np.cumsum([len(a) for _, _, a in chains])])
    q_len = [int(ms.reads.q_len[p]) for p, _, _ in chains]
    r_off, r_len, _, seq, shift = M.chain_windows_seqs(q_len, first, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat],
                                                       X.MAP_MARGIN, ms.seq_off, ms.seq_len)
    for c in range(len(chains)):
        s = int(seq[c])
        assert int(shift[c]) + int(r_len[c]) <= M.MAP_LENGTHS[s] and int(r_off[c]) == int(ms.seq_off[s]) + int(shift[c])
        assert ms.pool[int(r_off[c]):int(r_off[c]) + int(r_len[c])].tobytes() == ms.seqs[s][int(shift[c]):int(shift[c]) + int(r_len[c])]


def _paf_input():
    paf = dict(q_start=np.array([0, 5, 7]), q_end=np.array([90, 80, 60]), strand=np.array([b"+", b"-", b"+"], "S1"), t_start=np.array([10, 20, 30]),
               t_end=np.array([100, 95, 83]), n_match=np.array([85, 70, 50]), aln_len=np.array([92, 77, 55]), nm=np.array([7, 7, 5]),
               as_=np.array([150, 120, 90]))
    sel = dict(kept=np.array([0, 2, 1]), kept_first=np.array([0, 2, 3]), cls=np.array([0, 0, 1]), mapq=np.array([60, 40, 0]),
               sub_score=np.array([90, 0, 0]))
    return paf, sel


def test_paf_lines_with_a_target_per_chain(hip):
    paf, sel = _paf_input()
    sel["cls"] = np.array([hip.SEL_PRIMARY, hip.SEL_PRIMARY, hip.SEL_SECONDARY])
    names, lens = ["chr_a", b"contig_b", "chr_d"], [4000, 300, 6000]
    lines = hip.paf_lines(["r0", "r1"], [100, 90], names, lens, paf, sel, target=np.array([2, 0, 1], np.uint32))
    cols = [x.split("\t") for x in lines]
    assert [(c[0], c[5], c[6]) for c in cols] == [("r0", "chr_d", "6000"), ("r0", "contig_b", "300"), ("r1", "chr_a", "4000")]
    # without a target: today's lines, and with every chain on one target the same lines again
    plain = hip.paf_lines(["r0", "r1"], [100, 90], "chr_a", 4000, paf, sel, cigars=["90=", "75=", "53="])
    assert [x.split("\t")[5:7] for x in plain] == [["chr_a", "4000"]] * 3 and plain[0].endswith("cg:Z:90=")
    same = hip.paf_lines(["r0", "r1"], [100, 90], ["chr_a"], [4000], paf, sel, cigars=["90=", "75=", "53="], target=np.zeros(3, np.uint32))
    assert same == plain
    positional = hip.paf_lines(["r0", "r1"], [100, 90], "chr_a", 4000, paf, sel, ["90=", "75=", "53="])
    assert positional == plain
    with pytest.raises(ValueError, match="one entry per chain"):
        hip.paf_lines(["r0", "r1"], [100, 90], names, lens, paf, sel, target=[0, 1])
    with pytest.raises(ValueError, match="one entry per reference sequence"):
        hip.paf_lines(["r0", "r1"], [100, 90], names, lens, paf, sel, target=[0, 1, 3])
