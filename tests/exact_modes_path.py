"""Optimal alignment paths in a batch's own mode, in numpy / Python (test infrastructure; own code, written from the walk rules in
include/block_aligner_hip.h, "optimal paths in the batch's own mode"; no oracle/ and no reference code).

`matrices_mode` keeps every row of H, V and Z under the three start rules, `matrices_profile` every cell of T, Z, V and H of the profile
recurrence. `walk_mode`, `walk_profile` and `extend_paths` go backwards from an end cell by the rules and return (record, runs): the
record is (score, q_start, r_start, q_end, r_end, rows), the runs are packed as the library packs them (length << 4 | op; op 1 M, 2 =,
3 X, 4 I, 5 D), in alignment order and merged. `rescore_mode` and `rescore_profile` score a run list from its start cell, independently of
the matrices."""
from __future__ import annotations

import numpy as np

from block_aligner_amd.verify import _upper
from tests import exact_dp
from tests.exact_path import NEG, _table, images

GLOBAL, FREE_ROW0, LOCAL = "global", "free_query_start", "local"


def merged(ops_reversed):
    runs = []
    for op in reversed(ops_reversed):
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(n << 4) | op for op, n in runs]


def unpack(runs):
    return [(int(x) & 15, int(x) >> 4) for x in runs]


# ------------------------------------------------------------------ sequence matrices
def matrices_mode(q: bytes, r: bytes, matrix, gaps, start=GLOBAL):
    """-> (H, V, Z), int64 arrays of (|q| + 1, |r| + 1), under the start rule: GLOBAL (pure-gap borders), FREE_ROW0 (H[0][j] = 0) or LOCAL
    (H[0][j] = H[i][0] = 0 and H floored at 0). V and Z are "no cell" in row 0 and column 0."""
    tab = _table(matrix)
    qa, ra = images(q, r, matrix)
    nq, nr = len(qa), len(ra)
    o, e = int(gaps[0]), int(gaps[1])
    assert o <= e < 0
    jj = np.arange(nr + 1, dtype=np.int64)
    H = np.zeros((nq + 1, nr + 1), np.int64)
    V = np.full((nq + 1, nr + 1), NEG, np.int64)
    Z = np.full((nq + 1, nr + 1), NEG, np.int64)
    if start == GLOBAL:
        H[0, 1:] = o + (jj[1:] - 1) * e
    for i in range(1, nq + 1):
        H[i, 0] = 0 if start == LOCAL else o + (i - 1) * e
        if not nr:
            continue
        V[i, 1:] = np.maximum(H[i - 1, 1:] + o, V[i - 1, 1:] + e)
        T = np.empty(nr + 1, np.int64)               # the row without its horizontal gaps (floored, under LOCAL)
        T[0] = H[i, 0]
        T[1:] = np.maximum(H[i - 1, :-1] + tab[qa[i - 1], ra], V[i, 1:])
        if start == LOCAL:
            T = np.maximum(T, 0)
        Z[i, 1:] = np.maximum.accumulate(T - jj * e)[:-1] + o + (jj[1:] - 1) * e
        H[i, 1:] = np.maximum(T[1:], Z[i, 1:])
        assert (Z[i, 1:] == np.maximum(H[i, :-1] + o, Z[i, :-1] + e)).all()      # the recurrence as it is written
    return H, V, Z


def walk_mode(H, V, Z, qa, ra, tab, gaps, i: int, j: int, start=GLOBAL, eq: bool = False):
    """-> ((q_start, r_start), runs, ties): the walk from the end cell (i, j). ties counts the LOCAL stops at a cell whose diagonal also ties."""
    e = int(gaps[1])
    ops, state, ties = [], "H", 0
    while True:
        if state == "H":
            if start == LOCAL and H[i, j] == 0:
                if i and j and H[i - 1, j - 1] + tab[qa[i - 1], ra[j - 1]] == 0:
                    ties += 1
                break
            if i == 0 or j == 0:
                if start == FREE_ROW0 and i == 0:
                    break
                ops += [5] * j if i == 0 else [4] * i
                i = j = 0
                break
            if H[i, j] == H[i - 1, j - 1] + tab[qa[i - 1], ra[j - 1]]:
                ops.append((2 if qa[i - 1] == ra[j - 1] else 3) if eq else 1)
                i, j = i - 1, j - 1
            elif H[i, j] == V[i, j]:
                state = "V"
            else:
                assert H[i, j] == Z[i, j]
                state = "Z"
        elif state == "V":
            ops.append(4)
            state = "V" if V[i, j] == V[i - 1, j] + e else "H"
            i -= 1
        else:
            ops.append(5)
            state = "Z" if Z[i, j] == Z[i, j - 1] + e else "H"
            j -= 1
    return (i, j), merged(ops), ties


_cache = {}


def mode_paths(q: bytes, r: bytes, matrix, gaps, start=GLOBAL, free_query_end=False, what="global", x_drop=-1, eq=False, want_ties=False):
    """-> (record, runs) of ba_*_exact_paths on a sequence batch. The matrices of a pair and start rule are computed once and kept."""
    key = (q, r, id(matrix), tuple(gaps), start)
    ent = _cache.get(key)
    if ent is None:
        ent = _cache[key] = (matrix, matrices_mode(q, r, matrix, gaps, start))
    H, V, Z = ent[1]
    nq, nr = H.shape[0] - 1, H.shape[1] - 1
    if what == "extend":
        score, i, j, rows = exact_dp.extend_of(H, x_drop)
    elif free_query_end:
        j = int(np.argmax(H[nq]))
        score, i, rows = int(H[nq, j]), nq, nq + 1
    else:
        score, i, j, rows = int(H[nq, nr]), nq, nr, nq + 1
    qa, ra = images(q, r, matrix)
    (qs, rs), runs, ties = walk_mode(H, V, Z, qa, ra, _table(matrix), gaps, i, j, start, eq)
    rec = (score, qs, rs, i, j, rows)
    return (rec, runs, ties) if want_ties else (rec, runs)


def rescore_mode(runs, rec, q: bytes, r: bytes, matrix, gaps, eq=False):
    """The score of the runs from the record's start cell: the matrix per match-type column, open + (n - 1) extend per gap run. Checks that
    they consume exactly end - start and, with eq, that '=' / 'X' follow the image bytes. -> the score."""
    tab = _table(matrix)
    qa, ra = images(q, r, matrix)
    o, e = int(gaps[0]), int(gaps[1])
    _s, i, j, qe, re_, _rows = rec
    total, last = 0, 0
    for op, n in unpack(runs):
        assert n > 0 and op != last and op in ((2, 3, 4, 5) if eq else (1, 4, 5)), (op, n)
        last = op
        if op in (1, 2, 3):
            for _ in range(n):
                if op != 1:
                    assert (qa[i] == ra[j]) == (op == 2)
                total += int(tab[qa[i], ra[j]])
                i, j = i + 1, j + 1
        elif op == 4:
            total += o + (n - 1) * e
            i += n
        else:
            total += o + (n - 1) * e
            j += n
    assert (i, j) == (qe, re_), ((i, j), rec)
    return total


# ------------------------------------------------------------------ profiles
def _profile_arrays(q: bytes, profile):
    qa = _upper(np.frombuffer(q, np.uint8)).astype(np.int64) - 65
    sc = profile.pos_aa.astype(np.int64)
    oC, cC, oR = (np.asarray(x, np.int64) for x in (profile.pos_gap_open_C, profile.pos_gap_close_C, profile.pos_gap_open_R))
    return qa, sc, oC, cC, oR, int(profile.gap_extend)


def matrices_profile(q: bytes, profile):
    """-> (T, Z, V, H), int64 arrays of (|q| + 1, len(profile) + 1), of the header's profile recurrence; "no cell" is NEG."""
    qa, sc, oC, cC, oR, e = _profile_arrays(q, profile)
    nq, nr = len(qa), profile.str_len
    ii = np.arange(nq + 1, dtype=np.int64)
    T, Z, V, H = (np.full((nq + 1, nr + 1), NEG, np.int64) for _ in range(4))
    T[0, 0] = 0
    V[1:, 0] = oR[0] + ii[1:] * e
    H[:, 0] = np.maximum(T[:, 0], V[:, 0])
    for j in range(1, nr + 1):
        Z[:, j] = np.maximum(H[:, j - 1] + oC[j] + e, Z[:, j - 1] + e)
        t = Z[:, j] + cC[j]
        if nq:
            t[1:] = np.maximum(t[1:], H[:-1, j - 1] + sc[j, qa])
        T[:, j] = t
        if nq:   # V[i][j] = max over k < i of T[k][j] + oR[j] + (i - k) e
            V[1:, j] = np.maximum.accumulate(t - ii * e)[:-1] + oR[j] + ii[1:] * e
            assert (V[1:, j] == np.maximum(t[:-1] + oR[j] + e, V[:-1, j] + e)).all()
        H[:, j] = np.maximum(t, V[:, j])
    return T, Z, V, H


def walk_profile(T, Z, V, H, qa, sc, cC, e, i: int, j: int):
    """-> ((0, 0), runs, ties): ties = (cells visited in state H with T == V, cells visited in state T whose diagonal equals Z + close)."""
    ops, state = [], "H"
    t_eq_v = d_eq_z = 0
    while True:
        if state == "H":
            if j == 0:
                ops += [4] * i
                i = 0
                break
            t_eq_v += int(T[i, j] == V[i, j])
            state = "T" if H[i, j] == T[i, j] else "V"
        elif state == "T":
            if i == 0 and j == 0:
                break
            assert j >= 1
            diag = H[i - 1, j - 1] + sc[j, qa[i - 1]] if i >= 1 else None
            if diag is not None and T[i, j] == diag:
                d_eq_z += int(diag == Z[i, j] + cC[j])
                ops.append(1)
                i, j, state = i - 1, j - 1, "H"
            else:
                state = "Z"
        elif state == "Z":
            ops.append(5)
            state = "Z" if Z[i, j] == Z[i, j - 1] + e else "H"
            j -= 1
        else:
            assert i >= 1
            ops.append(4)
            state = "V" if V[i, j] == V[i - 1, j] + e else "T"
            i -= 1
    return (i, j), merged(ops), (t_eq_v, d_eq_z)


_pcache = {}


def profile_paths(q: bytes, profile, what="global", x_drop=-1, want_ties=False):
    """-> (record, runs) of ba_batch_exact_paths on a profile batch."""
    key = (q, id(profile))
    ent = _pcache.get(key)
    if ent is None:
        ent = _pcache[key] = (profile, matrices_profile(q, profile))
    T, Z, V, H = ent[1]
    qa, sc, _oC, cC, _oR, e = _profile_arrays(q, profile)
    nq, nr = H.shape[0] - 1, H.shape[1] - 1
    score, i, j, rows = exact_dp.extend_of(H, x_drop) if what == "extend" else (int(H[nq, nr]), nq, nr, nq + 1)
    (qs, rs), runs, ties = walk_profile(T, Z, V, H, qa, sc, cC, e, i, j)
    rec = (score, qs, rs, i, j, rows)
    return (rec, runs, ties) if want_ties else (rec, runs)


def rescore_profile(runs, rec, q: bytes, profile):
    """The score of the runs from (0, 0): s(j, q_i) per M column; a D run over positions j+1 .. j+n costs open_C[j+1] + n extend +
    close_C[j+n]; an I run of n residues after position j costs open_R[j] + n extend. -> the score."""
    qa, sc, oC, cC, oR, e = _profile_arrays(q, profile)
    _s, i, j, qe, re_, _rows = rec
    assert (i, j) == (0, 0)
    total, last = 0, 0
    for op, n in unpack(runs):
        assert n > 0 and op != last and op in (1, 4, 5), (op, n)
        last = op
        if op == 1:
            for _ in range(n):
                total += int(sc[j + 1, qa[i]])
                i, j = i + 1, j + 1
        elif op == 4:
            total += int(oR[j]) + n * e
            i += n
        else:
            total += int(oC[j + 1]) + n * e + int(cC[j + n])
            j += n
    assert (i, j) == (qe, re_), ((i, j), rec)
    return total


# ------------------------------------------------------------------ extension batches
def extend_paths(q: bytes, r: bytes, s: int, t: int, L: int, matrix, gaps, x_drop=-1, eq=False):
    """Seed (s, t, L) of the oriented query q against r -> (record, runs, left, right): the left side walked over the reversed prefixes
    and turned round, the seed's ungapped columns, the right side; left / right are the sides' (score, i, j, rows), zeros when empty."""
    from tests import exact_path
    tab = _table(matrix)

    def side(a, b):
        if not a or not b:
            return (0, 0, 0, 0), []
        return exact_path.exact_runs(a, b, matrix, gaps, "extend", x_drop, eq)

    left, lruns = side(q[:s][::-1], r[:t][::-1])
    right, rruns = side(q[s + L:], r[t + L:])
    qa, ra = images(q[s:s + L], r[t:t + L], matrix)
    seed_score = int(sum(tab[a, b] for a, b in zip(qa, ra)))
    cols = unpack(lruns)[::-1] + [(((2 if a == b else 3) if eq else 1), 1) for a, b in zip(qa, ra)] + unpack(rruns)
    runs = []
    for op, n in cols:
        if runs and runs[-1][0] == op:
            runs[-1][1] += n
        else:
            runs.append([op, n])
    rec = (left[0] + seed_score + right[0], s - left[1], t - left[2], s + L + right[1], t + L + right[2], left[3] + right[3])
    return rec, [(n << 4) | op for op, n in runs], left, right
