"""The numpy models of BA_EXACT_OWN_MODE (tests/exact_modes_dp.py) pinned without a GPU: against the independent DPs of tests/gotoh.py,
against their own cell-by-cell statements, and against the oracle with one block over the whole matrix -- the equalities the header
states for LOCAL_START, FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS (|q| < 16) and profile batches."""
import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import exact_dp, exact_modes_dp as M, gotoh
from tests.test_gotoh import AA20, _pow2_above, pos_profile_case

NUC = S.NucMatrix.new_simple(2, -3)
BYTES = S.ByteMatrix.new_simple(3, -2)
MODES = {"local_start": dict(local_start=True), "free_query_start_gaps": dict(free_query_start=True), "free_query_end_gaps": {}}


def dna_pair(rng, it, top):
    """A query inside the reference, unrelated heads on both, or a mutated copy: what the three modes are for."""
    L = int(rng.integers(1, top))
    r = synth.rand_str(rng, L, synth.DNA)
    if it % 3 == 0:
        a = int(rng.integers(0, L)); b = int(rng.integers(a, L)) + 1
        q = synth.mutate(rng, r[a:b], int(rng.integers(0, (b - a) // 5 + 1)), synth.DNA)
    elif it % 3 == 1:
        q = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 20)), synth.DNA), synth.mutate(rng, r, int(rng.integers(0, L // 6 + 1)), synth.DNA)])
        r = np.concatenate([synth.rand_str(rng, int(rng.integers(0, 20)), synth.DNA), r])
    else:
        q = synth.mutate(rng, r, int(rng.integers(0, L // 4 + 1)), synth.DNA)
    return q.tobytes(), r.tobytes()


@pytest.mark.parametrize("mode", sorted(MODES))
def test_last_rows_equal_gotoh(mode):
    rng = np.random.default_rng(71)
    kw = MODES[mode]
    for it in range(40):
        q, r = dna_pair(rng, it, (14, 60, 200)[it % 3])
        ge = -int(rng.integers(1, 4)); go = ge - int(rng.integers(0, 12))
        H = M.full_matrix_mode(q, r, NUC, (go, ge), **kw)
        want = gotoh.last_row_scores(q, r, NUC, (go, ge), local_start=kw.get("local_start", False), free_reference_start=kw.get("free_query_start", False))
        assert np.array_equal(H[len(q)], want), (mode, it)
        if mode == "free_query_end_gaps":
            assert np.array_equal(H, exact_dp.full_matrix(q, r, NUC, (go, ge)))        # the start rule is the global one
            s, i, j, rows = M.own_mode(H, "global", free_query_end=True)
            assert s == int(want.max()) and (i, rows) == (len(q), len(q) + 1) and j == int(np.flatnonzero(want == s)[0])


@pytest.mark.parametrize("matrix,gaps,alphabet", [(NUC, (-5, -1), synth.DNA), (S.static_matrix("BLOSUM62"), (-11, -1), synth.AMINO),
                                                  (BYTES, (-2, -2), np.arange(250, 256, dtype=np.uint8))])
def test_vectorised_modes_equal_the_cell_by_cell_statement(matrix, gaps, alphabet):
    rng = np.random.default_rng(72)
    pairs = [(synth.rand_str(rng, int(rng.integers(0, 40)), alphabet).tobytes(), synth.rand_str(rng, int(rng.integers(0, 40)), alphabet).tobytes())
             for _ in range(12)] + [(b"", b""), (b"", alphabet[:3].tobytes()), (alphabet[:3].tobytes(), b"")]
    if matrix is not BYTES:
        pairs[0] = (pairs[0][0].lower(), pairs[0][1])
    for q, r in pairs:
        for kw in ({}, dict(local_start=True), dict(free_query_start=True), dict(local_start=True, free_query_start=True)):
            H = M.full_matrix_mode(q, r, matrix, gaps, **kw)
            assert H.shape == (len(q) + 1, len(r) + 1)
            assert np.array_equal(H, M.full_matrix_mode_cells(q, r, matrix, gaps, **kw)), (q, r, kw)
            if kw.get("local_start"):
                assert H.min() >= 0 and not H[0].any() and not H[:, 0].any()
        assert np.array_equal(M.full_matrix_mode(q, r, matrix, gaps), exact_dp.full_matrix(q, r, matrix, gaps))


def uniform_profile(rng, L, B, go, ge):
    cons = bytes(AA20[i] for i in rng.integers(0, 20, L))
    p = S.AAProfile(L, B, ge)
    for i, c in enumerate(cons):
        for b in AA20:
            p.set(i + 1, b, S.BLOSUM62.get(c, b))
    for i in range(L + 1):
        p.set_gap_open_C(i, go); p.set_gap_close_C(i, 0); p.set_gap_open_R(i, go)
    q = synth.mutate(rng, np.frombuffer(cons, np.uint8), L // 3, np.frombuffer(AA20, np.uint8)).astype(np.uint8).tobytes()[: L + 30]
    return q, p


def test_profile_corners_equal_gotoh():
    rng = np.random.default_rng(73)
    for it in range(30):
        B = (16, 32, 64, 256)[it % 4]
        q, p = pos_profile_case(rng, B)
        H = M.full_matrix_profile(q, p)
        assert H.shape == (len(q) + 1, p.str_len + 1) and H[0, 0] == 0
        assert int(H[-1, -1]) == gotoh.global_score_profile_pos(q, p), (it, B)
        if B <= 32:
            assert np.array_equal(H, M.full_matrix_profile_cells(q, p)), (it, B)
    for it in range(12):
        go = -int(rng.integers(5, 14))
        q, p = uniform_profile(rng, int(rng.integers(1, (14, 60, 200)[it % 3])), 256, go, -1)
        assert int(M.full_matrix_profile(q, p)[-1, -1]) == gotoh.global_score_profile(q, p, go), it
    # an empty query, and positions that were never set (-128 everywhere) are taken as they are
    q, p = pos_profile_case(rng, 32)
    assert int(M.full_matrix_profile(b"", p)[0, -1]) == gotoh.global_score_profile_pos(b"", p)
    tail = S.AAProfile(p.str_len + 5, 32, p.gap_extend)
    tail.pos_aa[: p.str_len + 1] = p.pos_aa[: p.str_len + 1]
    for dst, src in ((tail.pos_gap_open_C, p.pos_gap_open_C), (tail.pos_gap_close_C, p.pos_gap_close_C), (tail.pos_gap_open_R, p.pos_gap_open_R)):
        dst[: p.str_len + 1] = src[: p.str_len + 1]
    Ht = M.full_matrix_profile(q, tail)
    assert np.array_equal(Ht[:, : p.str_len + 1], M.full_matrix_profile(q, p)) and np.array_equal(Ht, M.full_matrix_profile_cells(q, tail))
    assert int(Ht[-1, -1]) == gotoh.global_score_profile_pos(q, tail) < int(Ht[-1, p.str_len])


@pytest.mark.parametrize("mode", ["local_start", "free_query_start_gaps"])
def test_oracle_with_one_block_equals_own_mode_global(oracle, mode):
    rng = np.random.default_rng(74)
    for it in range(30):
        q, r = dna_pair(rng, it, (14, 60, 200)[it % 3])
        if not q:
            continue
        ge = -int(rng.integers(1, 4)); go = ge - int(rng.integers(1, 12))
        B = _pow2_above(max(len(q), len(r)))
        res = oracle.align(NUC, q, r, (go, ge), (B, B), 0, (mode,))
        want = M.own_mode(M.full_matrix_mode(q, r, NUC, (go, ge), **MODES[mode]), "global")
        assert (res["score"], res["query_idx"], res["reference_idx"]) == want[:3], (mode, it)


def test_oracle_with_one_block_equals_own_mode_global_for_profiles(oracle):
    rng = np.random.default_rng(75)
    for B in (16, 64, 256):
        for it in range(10):
            q, p = pos_profile_case(rng, B)
            res = oracle.align_profile(q, p, (B, B), 0, ())
            assert res["score"] == M.own_mode(M.full_matrix_profile(q, p), "global")[0], (B, it)


def test_oracle_free_query_end_gaps_short_queries(oracle):
    """|q| < 16 with one block over the matrix: the reported score is max(exact, 0) -- the lane rule reads the last query row and padded
    rows only, and starts at 0."""
    rng = np.random.default_rng(76)
    negative = 0
    for it in range(40):
        r = synth.rand_str(rng, int(rng.integers(1, 120)), synth.DNA)
        nq = int(rng.integers(1, 16))
        if it % 2:
            a = int(rng.integers(0, len(r)))
            q = synth.mutate(rng, r[a:a + nq], int(rng.integers(0, 3)), synth.DNA)
        else:
            q = synth.rand_str(rng, nq, synth.DNA)
        if len(q) == 0:
            continue
        ge = -int(rng.integers(1, 4)); go = ge - int(rng.integers(1, 12))
        m = S.NucMatrix.new_simple(int(rng.integers(1, 4)), -int(rng.integers(1, 5))) if it % 4 else S.NucMatrix.new_simple(1, -9)
        B = _pow2_above(max(len(q), len(r)))
        res = oracle.align(m, q.tobytes(), r.tobytes(), (go, ge), (B, B), 0, ("free_query_end_gaps",))
        exact = M.own_mode(M.full_matrix_mode(q.tobytes(), r.tobytes(), m, (go, ge)), "global", free_query_end=True)[0]
        negative += exact < 0
        assert res["score"] == max(exact, 0), (it, len(q), len(r), res["score"], exact)
    assert negative >= 1


def small_range_profile(rng, form):
    """A PSSM of 20 .. 300 positions in a 64-cell block and a related query: "uniform" gap costs (open_C = open_R, close_C = 0) or
    position-"specific" ones, as tests/test_gpu_exact_modes.py draws them."""
    nq, nr = int(rng.integers(20, 300)), int(rng.integers(20, 300))
    aa = np.frombuffer(AA20, np.uint8)
    cons = aa[rng.integers(0, 20, nr)]
    p = S.AAProfile(nr, 64, -1)
    for i, c in enumerate(cons):
        for a in aa:
            p.set(i + 1, int(a), S.BLOSUM62.get(int(c), int(a)))
    go = int(rng.integers(-12, -4))
    for i in range(nr + 1):
        if form == "uniform":
            p.set_gap_open_C(i, go); p.set_gap_close_C(i, 0); p.set_gap_open_R(i, go)
        else:
            p.set_gap_open_C(i, int(rng.integers(-14, -3))); p.set_gap_open_R(i, int(rng.integers(-14, -3))); p.set_gap_close_C(i, int(rng.integers(-4, 1)))
    q = np.concatenate([synth.mutate(rng, cons, nr // 8, aa), synth.rand_str(rng, nq, aa)])[:nq].astype(np.uint8).tobytes()
    return q, p


def test_small_block_range_never_exceeds_the_profile_definition_for_uniform_costs(oracle):
    """The header's bound for profile batches: with position-independent gap costs a 32..64 run never scores above OWN_MODE GLOBAL."""
    rng = np.random.default_rng(77)
    for it in range(30):
        q, p = small_range_profile(rng, "uniform")
        res = oracle.align_profile(q, p, (32, 64), 0, ())
        assert res["score"] <= M.own_mode(M.full_matrix_profile(q, p), "global")[0], (it, len(q), p.str_len)


def test_small_block_range_can_exceed_the_profile_definition_for_specific_costs(oracle):
    """... and why the header restricts it: with position-specific costs the reference's own 32..64 result lies above the definition's
    optimum on some pairs, by a few points (rectangles along the profile state another recurrence). A known property, pinned here so
    that the header's wording stays under test."""
    rng = np.random.default_rng(78)
    above = []
    for it in range(30):
        q, p = small_range_profile(rng, "specific")
        res = oracle.align_profile(q, p, (32, 64), 0, ())
        ex = M.own_mode(M.full_matrix_profile(q, p), "global")[0]
        if res["score"] > ex:
            above.append(res["score"] - ex)
        B = 512                                                   # one block over the matrix: equality, for any costs
        big = S.AAProfile(p.str_len, B, -1)
        big.pos_aa[: p.str_len + 1] = p.pos_aa[: p.str_len + 1]
        for dst, src in ((big.pos_gap_open_C, p.pos_gap_open_C), (big.pos_gap_close_C, p.pos_gap_close_C), (big.pos_gap_open_R, p.pos_gap_open_R)):
            dst[: p.str_len + 1] = src[: p.str_len + 1]
        assert oracle.align_profile(q, big, (B, B), 0, ())["score"] == ex, it
    assert above, "the 32..64 oracle no longer exceeds the definition: the header's bound can be stated for every profile"
