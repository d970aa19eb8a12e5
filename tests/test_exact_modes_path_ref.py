"""The path model of tests/exact_modes_path.py on the CPU: its runs rescore to the scores of tests/exact_modes_dp.py, consume exactly
end - start, local starts sit on H == 0, plain mode reproduces tests/exact_path.py run for run, and the tie rules of the walk are
exercised by the tie-heavy inputs (asserted here: otherwise the inputs would be wrong)."""
import functools

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import exact_modes_dp as M, exact_modes_path as P, exact_path

NUC = S.NucMatrix.new_simple(1, -1)
GAPS = (-2, -1)
STARTS = {P.GLOBAL: {}, P.FREE_ROW0: dict(free_query_start=True), P.LOCAL: dict(local_start=True)}
SHAPES = ((1, 1), (1, 9), (9, 1), (15, 63), (64, 65), (65, 64), (40, 120), (129, 70))
AA = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", np.uint8)


@functools.lru_cache(maxsize=None)
def tie_pairs():
    """Two-letter sequences under +1 / -1 with gaps (-2, -1): nearly every cell ties somewhere."""
    rng = np.random.default_rng(700)
    two = np.frombuffer(b"AC", np.uint8)
    return tuple((synth.rand_str(rng, nq, two).tobytes(), synth.rand_str(rng, nr, two).tobytes()) for nq, nr in SHAPES + ((30, 30),) * 6)


def tie_profile(rng, nq, nr, ge=-1):
    """A two-residue profile with scores +1 / -1, open_C = open_R = -1, close_C in {0, -1}: T == V and diagonal == Z + close both occur."""
    p = S.AAProfile(nr, 512, ge)
    cons = rng.integers(0, 2, nr)
    for i in range(nr):
        for a in AA:
            p.set(i + 1, int(a), 1 if a == AA[cons[i]] else -1)
    for i in range(nr + 1):
        p.set_gap_open_C(i, -1); p.set_gap_open_R(i, -1); p.set_gap_close_C(i, -int(rng.integers(0, 2)))
    return AA[rng.integers(0, 2, nq)].tobytes(), p


@functools.lru_cache(maxsize=None)
def tie_profiles():
    rng = np.random.default_rng(701)
    return tuple(tie_profile(rng, nq, nr) for nq, nr in SHAPES + ((30, 30),) * 6)


@pytest.mark.parametrize("start", list(STARTS))
@pytest.mark.parametrize("free_end", [False, True])
def test_sequence_paths_rescore_to_the_own_mode_scores(start, free_end):
    ties = 0
    for q, r in tie_pairs():
        H = M.full_matrix_mode(q, r, NUC, GAPS, **STARTS[start])
        for what, x in (("global", -1), ("extend", -1), ("extend", 0), ("extend", 3)):
            for eq in (False, True):
                rec, runs, t = P.mode_paths(q, r, NUC, GAPS, start, free_end, what, x, eq, want_ties=True)
                ties += t
                assert (rec[0], rec[3], rec[4], rec[5]) == M.own_mode(H, what, x, free_end)
                assert P.rescore_mode(runs, rec, q, r, NUC, GAPS, eq) == rec[0]     # (also: the runs consume exactly end - start)
                if start == P.LOCAL:
                    assert H[rec[1], rec[2]] == 0
                elif start == P.GLOBAL:
                    assert rec[1:3] == (0, 0)
                else:
                    assert rec[1] == 0
    if start == P.LOCAL:
        assert ties > 0      # a stop cell that also ties on the diagonal


def test_plain_mode_reproduces_exact_path():
    for q, r in tie_pairs():
        for what, x in (("global", -1), ("extend", -1), ("extend", 3)):
            for eq in (False, True):
                rec, runs = P.mode_paths(q, r, NUC, GAPS, P.GLOBAL, False, what, x, eq)
                rec0, runs0 = exact_path.exact_runs(q, r, NUC, GAPS, what, x, eq)
                assert runs == runs0 and (rec[0], rec[3], rec[4], rec[5]) == rec0 and rec[1:3] == (0, 0)


def test_profile_paths_rescore_to_the_own_mode_scores():
    t_eq_v = d_eq_z = 0
    for q, p in tie_profiles():
        H = M.full_matrix_profile(q, p)
        assert np.array_equal(P.matrices_profile(q, p)[3], H)
        for what, x in (("global", -1), ("extend", -1), ("extend", 0), ("extend", 3)):
            rec, runs, t = P.profile_paths(q, p, what, x, want_ties=True)
            t_eq_v += t[0]; d_eq_z += t[1]
            assert (rec[0], rec[3], rec[4], rec[5]) == M.own_mode(H, what, x) and rec[1:3] == (0, 0)
            assert P.rescore_profile(runs, rec, q, p) == rec[0]
    assert t_eq_v > 0 and d_eq_z > 0


def test_extend_paths_rescore():
    rng = np.random.default_rng(702)
    m, gaps = S.NucMatrix.new_simple(2, -3), (-5, -1)
    for n in range(12):
        r = synth.rand_str(rng, 120, synth.DNA)
        q = synth.mutate(rng, r, 10, synth.DNA).tobytes()
        r = r.tobytes()
        s, t, L = (0, 0, 8) if n == 0 else (len(q) - 8, len(r) - 8, 8) if n == 1 else (50, 50, 10)
        for eq in (False, True):
            rec, runs, left, right = P.extend_paths(q, r, s, t, L, m, gaps, -1, eq)
            assert P.rescore_mode(runs, rec, q, r, m, gaps, eq) == rec[0]
            assert rec[5] == left[3] + right[3]


# ---------------------------------------------------------------- the use case of tests/test_gpu_exact_paths.py, on the CPU first
RESCUE_NUC, RESCUE_GAPS, RESCUE_SIZE = S.NucMatrix.new_simple(2, -3), (-5, -1), (32, 64)


@functools.lru_cache(maxsize=None)
def rescue_pairs():
    """32 pairs of a 95-letter reference and a mutated copy; every other query carries a 200-letter random insertion in its middle, which
    a block range of 32 .. 64 cannot span. Every pair is below 300 x 300."""
    rng = np.random.default_rng(341)
    lists = []
    for n in range(32):
        base = synth.rand_str(rng, 95, synth.DNA)
        q = synth.mutate(rng, base, 3, synth.DNA)
        if n % 2:
            q = np.concatenate([q[:45], synth.rand_str(rng, 200, synth.DNA), q[45:]])
        lists.append((q.tobytes(), base.tobytes()))
    return tuple(lists)


def test_rescue_construction_takes_a_small_block_range_off_the_optimum(oracle):
    """The CPU restatement of the block aligner at 32 .. 64 in LOCAL_START against the exact LOCAL_START optimum of the model: some of the
    pairs with the insertion score below it, and no pair scores above."""
    below = 0
    for n, (q, r) in enumerate(rescue_pairs()):
        rec, runs = P.mode_paths(q, r, RESCUE_NUC, RESCUE_GAPS, P.LOCAL)
        assert rec[0] == M.own_mode(M.full_matrix_mode(q, r, RESCUE_NUC, RESCUE_GAPS, local_start=True), "global")[0]
        got = oracle.align(RESCUE_NUC, q, r, RESCUE_GAPS, RESCUE_SIZE, 0, ("local_start",))
        assert got["score"] <= rec[0], n
        if got["score"] < rec[0]:
            below += 1
            assert n % 2, n      # only a pair with the insertion
    assert below > 0
