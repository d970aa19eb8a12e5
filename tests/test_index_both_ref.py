"""The model of seeding both strands at once (tests/index_both_ref.py) on the CPU: the known answers of INTEGRATION.md, "Both strands at
once", the plain rule against its NumPy form, what follows from the rule -- the tie to today's indexed seeder for odd k, the palindromes
that make the difference for even k, strand symmetry at w = 1 --, and that the cases of tests/test_gpu_index_both.py tell the rule from
its neighbouring mistakes."""
import numpy as np
import pytest

from tests import index_both_ref as B, index_ref as X, seeding_ref as S


def pairs(p):
    return list(zip(p["q_hit"].tolist(), p["r_hit"].tolist()))


def same(reads, seqs, P):
    """hits() against hits_plain() for every read; entries() against entries_plain() -> the number of hits."""
    code, pos, longest = B.entries(seqs, P.k, P.w)
    plain = B.entries_plain(seqs, P.k, P.w)
    assert list(zip(code.tolist(), (pos >> 31).tolist(), (pos & B.POS_MASK).tolist())) == plain
    runs = {}
    for c, _, _ in plain:
        runs[c] = runs.get(c, 0) + 1
    assert longest == max(runs.values(), default=0)
    total = 0
    for r, e in zip(reads, B.expected(reads, seqs, P)):
        sk = B.sketch_plain(r, P.k, P.w)
        assert list(zip((e["q_pos"] & B.POS_MASK).tolist(), e["q_code"].tolist(), (e["q_pos"] >> 31).tolist())) == sk
        plus, minus = B.hits_plain(r, seqs, P)
        assert pairs(e["problems"][0]) == plus and pairs(e["problems"][1]) == minus
        total += len(plus) + len(minus)
    return total


# ------------------------------------------------------------------ known answers
KNOWN_R_SKETCH = [(1, 108, 1), (5, 912, 1), (6, 228, 1), (10, 724, 1), (11, 437, 1), (13, 108, 0), (16, 808, 0), (17, 163, 0), (21, 488, 1),
                  (22, 122, 1), (24, 180, 0), (26, 440, 1), (29, 262, 1), (31, 912, 1)]
KNOWN_Q_SKETCH = [(3, 912, 1), (4, 228, 1), (8, 724, 1), (10, 173, 1), (11, 92, 0), (12, 370, 0), (13, 370, 1), (14, 808, 0), (15, 163, 0),
                  (19, 488, 1), (20, 122, 1), (26, 27, 1), (27, 262, 1), (29, 912, 1), (30, 228, 1)]
KNOWN_Q_PLUS = [(3, 5), (29, 5), (4, 6), (30, 6), (8, 10), (14, 16), (15, 17), (19, 21), (20, 22), (27, 29), (3, 31), (29, 31)]
KNOWN_Q_MINUS_SKETCH = [(2, 313, 0), (3, 228, 0), (4, 912, 0), (6, 262, 0), (7, 27, 0), (13, 122, 0), (14, 488, 0), (16, 565, 1)]
KNOWN_Q_MINUS_MINUS = [(11, 3), (13, 5), (14, 6), (15, 7), (3, 21), (4, 22), (11, 29), (13, 31)]


def test_the_known_answers_position_by_position():
    assert B.sketch_plain(S.KNOWN_R, 5, 4) == KNOWN_R_SKETCH
    assert B.sketch_plain(S.KNOWN_Q, 5, 4) == KNOWN_Q_SKETCH
    plus, minus = B.hits_plain(S.KNOWN_Q, [S.KNOWN_R], B.Params(5, 4, 2, B.NO_CAP))
    assert plus == KNOWN_Q_PLUS and minus == []
    assert B.sketch_plain(S.KNOWN_Q_MINUS, 5, 3) == KNOWN_Q_MINUS_SKETCH
    plus, minus = B.hits_plain(S.KNOWN_Q_MINUS, [S.KNOWN_R], B.Params(5, 3, 4, B.NO_CAP))
    assert plus == [(16, 18)] and minus == KNOWN_Q_MINUS_MINUS
    # three codes occur twice in the index at w = 3: a reference cap of 1 takes their hits
    index = B.entries_plain([S.KNOWN_R], 5, 3)
    twice = sorted(c for c in {c for c, _, _ in index} if sum(1 for c2, _, _ in index if c2 == c) > 1)
    assert twice == [108, 262, 912]   # (the read holds 262 at 6 and 912 at 4, and not 108: the four hits that go are theirs)

    plus, minus = B.hits_plain(S.KNOWN_Q_MINUS, [S.KNOWN_R], B.Params(5, 3, 4, 1))
    assert plus == [(16, 18)] and minus == [(14, 6), (15, 7), (3, 21), (4, 22)]


def test_the_known_answers_in_numpy():
    for reads, P in (([S.KNOWN_Q, S.KNOWN_Q_MINUS, b"ACGNACGNNACG", b"", b"CCCCCCCCCCCCC"], B.Params(5, 4, 2, B.NO_CAP)),
                     ([S.KNOWN_Q, S.KNOWN_Q_MINUS], B.Params(5, 3, 4, B.NO_CAP)), ([S.KNOWN_Q, S.KNOWN_Q_MINUS], B.Params(5, 3, 4, 1))):
        assert same(reads, [S.KNOWN_R], P) > 0
    e = B.hits(S.KNOWN_Q, [S.KNOWN_R], B.Params(5, 4, 2, B.NO_CAP))
    assert pairs(e["problems"][0]) == KNOWN_Q_PLUS and pairs(e["problems"][1]) == []


def test_canonical_codes_by_hand():
    # ACGTT: f = 0b0001101111 = 111; its reverse complement AACGT: g = 0b0000011011 = 27 -> code 27, strand 1
    assert B.canon_plain(b"ACGTT", 5) == [(27, 1)] and B.canon_plain(b"AACGT", 5) == [(27, 0)]
    assert B.canon_plain(b"ACGT", 4) == [None] and B.canon_plain(b"ACGT", 4, "palindrome_kept") == [(27, 0)]   # its own reverse complement
    assert B.canon_plain(b"acNgt", 2) == [(1, 0), None, None, (1, 1)]
    assert B.canon_plain(b"T" * 16, 16) == [(0, 1)] and B.canon_plain(b"A" * 16, 16) == [(0, 0)]
    assert B.is_palindrome(b"GAATTC") and not B.is_palindrome(b"GAATTG")


# ------------------------------------------------------------------ plain against NumPy
@pytest.mark.parametrize("k, w", [(4, 1), (6, 5), (15, 10), (16, 64)])
def test_plain_equals_numpy_on_random_sequences(k, w):
    rng = np.random.default_rng(3 + 100 * k + w)
    for _ in range(8):
        seqs = [S.dna(rng, int(n)) for n in rng.integers(0, 300, 3)]
        base = b"".join(seqs)
        reads = [S.mutate(rng, base[a:a + 150], 0.05) for a in (0, 100, 300)] + [B.revcomp(S.mutate(rng, base[50:260], 0.05)), S.dna(rng, 80), b""]
        same(reads, seqs, B.Params(k, w, int(rng.integers(1, 5)), int(rng.integers(1, 5))))
        same(reads, seqs, B.Params(k, w, B.NO_CAP, B.NO_CAP))


# ------------------------------------------------------------------ what follows from the rule
@pytest.mark.parametrize("k", [5, 7, 15])
def test_for_odd_k_without_windows_and_caps_the_problems_are_the_indexed_seeders(k):
    """Problem 2 r + s has exactly the hits of index_ref.hits_plain for read r listed on strand s."""
    rng = np.random.default_rng(200 + k)
    P = B.Params(k, 1, B.NO_CAP, B.NO_CAP)
    n_hits = 0
    for case in range(20):
        ref = S.dna(rng, int(rng.integers(40, 300)))
        a = int(rng.integers(0, len(ref) - 30))
        read = S.mutate(rng, ref[a:a + int(rng.integers(20, 120))], 0.05)
        if case % 3 == 0 and len(read) > 12:
            read = read[:10] + b"N" + read[11:]
        if case % 2:
            read = B.revcomp(read)
        got = B.hits_plain(read, [ref], P)
        for s in (0, 1):
            assert got[s] == X.hits_plain(read, ref, P, s), (case, s)
            n_hits += len(got[s])
    assert n_hits > 100


@pytest.mark.parametrize("k", [4, 6, 12])
def test_for_even_k_the_difference_is_exactly_the_palindromes(k):
    rng = np.random.default_rng(300 + k)
    P = B.Params(k, 1, B.NO_CAP, B.NO_CAP)
    dropped = 0
    for case in range(12):
        ref = S.dna(rng, 200) + b"ACGT" * 4 + S.dna(rng, 60) + b"GAATTC" * 3
        read = S.mutate(rng, ref[20:], 0.03)
        if case % 2:
            read = B.revcomp(read)
        got = B.hits_plain(read, [ref], P)
        for s in (0, 1):
            want = X.hits_plain(read, ref, P, s)
            keep = [(q, r) for q, r in want if not B.is_palindrome(ref[r:r + k])]
            assert got[s] == keep, (case, s)
            assert all(B.is_palindrome(S.oriented(read, s)[q:q + k]) for q, r in want if (q, r) not in keep)
            dropped += len(want) - len(keep)
    assert dropped > 0


@pytest.mark.parametrize("k", [5, 8, 16])
def test_strand_symmetry_without_windows(k):
    """Seeding revcomp(read) swaps the two problems' hit lists, at w = 1 (with windows leftmost becomes rightmost: no claim)."""
    rng = np.random.default_rng(400 + k)
    for caps in ((B.NO_CAP, B.NO_CAP), (2, 3)):
        P = B.Params(k, 1, *caps)
        for _ in range(10):
            ref = S.dna(rng, 300)
            read = S.mutate(rng, ref[40:200], 0.05) + B.revcomp(ref[210:280])
            a, b = B.hits_plain(read, [ref[:150], ref[150:]], P), B.hits_plain(B.revcomp(read), [ref[:150], ref[150:]], P)
            assert a[0] == b[1] and a[1] == b[0] and a[0] and a[1]


# ------------------------------------------------------------------ the cases of the GPU tests
def differs(seqs, reads, P, mistake) -> bool:
    if B.entries_plain(seqs, P.k, P.w) != B.entries_plain(seqs, P.k, P.w, mistake):
        return True
    return any(B.hits_plain(r, seqs, P) != B.hits_plain(r, seqs, P, mistake) or B.sketch_plain(r, P.k, P.w) != B.sketch_plain(r, P.k, P.w, mistake)
               for r in reads)


@pytest.mark.parametrize("k, w", B.INDEX_KW)
def test_the_index_cases_are_what_they_say(k, w):
    cases = B.index_cases(k, w)
    for nw in B.SEAM_WINDOWS:
        seq, = cases[f"random_{nw}"]
        assert len(seq) - k + 1 - w + 1 == nw
    for name, seqs in cases.items():
        code, pos, longest = B.entries(seqs, k, w)
        if name.startswith("random") or name == "four_sequences":
            plain = B.entries_plain(seqs, k, w)
            assert list(zip(code.tolist(), (pos >> 31).tolist(), (pos & B.POS_MASK).tolist())) == plain, name
        assert len(code) > 0 and set((pos >> 31).tolist()) == {0, 1}, name
    # the strand bit in the order key would select other k-mers where a window holds a code on both strands
    if w > 1:
        assert differs(cases["inverted_repeats"], [], B.Params(k, w, 1, 1), "strand_in_order_key")
    if k % 2 == 0:   # a palindrome kept would be an entry
        if k != 6:   # (at k = 6, w = 5 the repeat's palindromes CGTACG and TACGTA are no window's minimum, kept or not)
            assert differs(cases["acgt_repeats"], [], B.Params(k, w, 1, 1), "palindrome_kept")
        assert differs(cases["inverted_repeats"], [], B.Params(k, w, 1, 1), "palindrome_kept")
    if k == 4:
        code, pos, _ = B.entries(cases["acgt_repeats"], k, w)
        assert sorted(set(code.tolist())) == [min(S.codes_plain(x, 4)[0], S.codes_plain(B.revcomp(x), 4)[0]) for x in (b"CGTA",)]
    # no entry lies over a junction, and the k-mer that straddles the first one matches nothing
    seqs = cases["four_sequences"]
    start = [0]
    for s in seqs:
        start.append(start[-1] + len(s))
    p = (B.entries(seqs, k, w)[1] & B.POS_MASK).astype(np.int64)
    for lo, hi in zip(start, start[1:]):
        assert not ((p < hi) & (p + k > hi) & (p >= lo)).any()
    if k >= 15:   # (a shorter k-mer occurs elsewhere by chance)
        x_code = B.canon_plain(seqs[0][-(k // 2):] + seqs[1][:k - k // 2], k)[0][0]
        assert (B.entries([b"".join(seqs)], k, 1)[0] == x_code).sum() == 2
        assert (B.entries(seqs, k, 1)[0] == x_code).sum() == 1   # only its reverse complement, inside sequence 3


@pytest.mark.parametrize("k, w", B.INDEX_KW)
def test_the_read_cases_are_what_they_say(k, w):
    seqs, rs = B.read_cases(k, w)
    assert [len(q) for q in rs.reads[:3]] == [0, k - 1, k]
    for q, nw in zip(rs.reads[3:], B.READ_WINDOWS):
        assert len(q) - k + 1 - w + 1 == nw
    P = B.Params(k, w, 8, 8)
    assert same(rs.reads, seqs, P) > 0
    exps = B.expected(rs.reads, seqs, P)
    assert [len(e["q_pos"]) for e in exps[:2]] == [0, 0]
    assert sum(len(e["problems"][0]["q_hit"]) for e in exps) > 0 and sum(len(e["problems"][1]["q_hit"]) for e in exps) > 0
    assert differs(seqs, rs.reads, P, "minus_q_off_by_k")
    if w > 1:
        assert differs(seqs, rs.reads, P, "strand_in_order_key")
    if k % 2 == 0:   # (k = 16 included: the shape where g is made with a shift of 0)
        assert differs(seqs, rs.reads, P, "palindrome_kept")


def test_the_strands_case_is_what_it_says():
    seqs, rs = B.strands_case()
    P = B.Params(11, 3, 8, 8)
    assert same(rs.reads, seqs, P) > 0
    e = B.expected(rs.reads, seqs, P)
    assert len(e[0]["q_pos"]) > 128
    # every step of 64 sorted entries of the first read has hits of both problems
    both = B.hits_plain(rs.reads[0], seqs, P)
    order = sorted(B.sketch_plain(rs.reads[0], P.k, P.w), key=lambda x: (x[1], x[2], x[0]))
    n = len(rs.reads[0])
    for a in range(0, len(order) - 63, 64):
        own = {i for i, _, _ in order[a:a + 64]}
        assert any(q in own for q, _ in both[0]) and any(n - P.k - q in own for q, _ in both[1]), a
    assert [len(p["q_hit"]) > 0 for x in e[1:] for p in x["problems"]] == [False, True, False, False]
    assert differs(seqs, rs.reads, P, "minus_q_off_by_k")


@pytest.mark.parametrize("max_occ, max_ref_occ", B.OCC_CAPS)
def test_the_occ_cases_are_what_they_say(max_occ, max_ref_occ):
    for k in (13, 16):
        seqs, rs = B.occ_case(k, max_occ, max_ref_occ)
        P = B.Params(k, 1, max_occ, max_ref_occ)
        same(rs.reads, seqs, P)
        plus, minus = B.hits_plain(rs.reads[0], seqs, P)
        assert len(plus) + len(minus) == max_occ * max_ref_occ   # the group at both caps stays, the three over either go
        assert (max_occ * max_ref_occ == 1) == (minus == [])       # ... and its entries are split across the strands
        over = B.hits_plain(rs.reads[0], seqs, B.Params(k, 1, max_occ + 1, max_ref_occ + 1))
        assert len(over[0]) + len(over[1]) == max_occ * max_ref_occ + (max_occ + 1) * max_ref_occ + max_occ * (max_ref_occ + 1) + (max_occ + 1) * (max_ref_occ + 1)
        assert differs(seqs, rs.reads, P, "caps_per_strand")
        a, b = B.hits_plain(rs.reads[1], seqs, P)   # the reverse complement of the read: the problems swapped (w = 1)
        assert (a, b) == (minus, plus)


@pytest.mark.parametrize("extra", [0, 1])
def test_the_hit_sort_case_is_what_it_says(extra):
    seqs, rs = B.hit_sort_case(extra)
    for ref_occ, big in ((128, X.SORT_LDS + extra), (127, extra)):
        exps = B.per_problem(B.expected(rs.reads, seqs, B.Params(12, 1, 64, ref_occ)))
        assert [len(p["q_hit"]) for p in exps] == [0, 0, 1, 0, 0, big, 2, 0]
    P = B.Params(12, 1, 64, 128)
    assert B.hits_plain(rs.reads[1], seqs, P) == tuple(pairs(p) for p in exps[2:4])
    assert differs(seqs, rs.reads[2:3], P, "minus_q_off_by_k")


@pytest.mark.parametrize("k", [5, 11, 15])
def test_the_tie_case_equals_the_listed_twice_model(k):
    seqs, rs = B.tie_case(k)
    P = B.Params(k, 1, B.NO_CAP, B.NO_CAP)
    got = B.per_problem(B.expected(rs.reads, seqs, P))
    twice = rs.listed_twice()
    assert len(twice) == len(got) and twice.strand.tolist() == [0, 1] * len(rs)
    from tests import index_multi_ref as M
    minus_hits = 0
    for p, (q, s) in enumerate(twice.reads):
        want = M.hits_multi(q, seqs, P, s)
        assert np.array_equal(got[p]["q_hit"], want["q_hit"]) and np.array_equal(got[p]["r_hit"], want["r_hit"]), p
        minus_hits += s * len(want["q_hit"])
    assert minus_hits > 0 and any(b"N" in q for q in rs.reads)


def test_the_mapping_set_places_every_read_by_the_model_alone():
    """The read set of the whole path: the model's rank-0 chain of every read's true problem lies on the read's own sequence, over the
    interval it was drawn from, and outscores every chain of the other strand; the chimeric read has a chain on each of its two sequences."""
    from tests import index_multi_ref as M
    ms = B.BothMappingSet()
    assert len(ms.once) == B.MAP_READS and all(1000 <= len(q) <= 2200 for q in ms.once.reads) and sum(B.MAP_LENGTHS) == 20000
    assert sum(o[3] for o in ms.origin) == len(ms.origin) // 2
    exps = ms.expected_hits()
    assert len(exps) == 2 * B.MAP_READS
    chains = M.model_chains(exps, ms.start, X.MAP_CHAINING, B.MAP_PARAMS.k)
    best = {}
    for p, rank, anchors in chains:
        best.setdefault(p, []).append((rank, anchors))
    for i, (s, lo, hi, strand) in enumerate(ms.origin):
        anchors = dict(best[ms.true_problem(i)])[0]
        r0, r1 = anchors[0][1], anchors[-1][1] + anchors[-1][2]
        assert ms.start[s] + lo <= r0 + 50 and r1 <= ms.start[s] + hi + 50 and r1 - r0 > (hi - lo) // 2, i
        assert M.seq_of(ms.start, r0) == s
        other = dict(best.get(2 * i + 1 - strand, []))
        assert sum(g for _, _, g in anchors) > 3 * sum(g for _, _, g in other.get(0, [])), i
    two = [a for _, a in best[2 * ms.chimeric]][:2]
    assert sorted(M.seq_of(ms.start, a[0][1]) for a in two) == [1, 3]
