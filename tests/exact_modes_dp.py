"""Full-matrix DP of small pairs in a batch's own mode, in numpy (test infrastructure; own code, written from the definitions in
include/block_aligner_hip.h, "exact scores in the batch's own mode"; no oracle/ and no reference code).

`full_matrix_mode` is tests/exact_dp.py's `full_matrix` with the start rules of BA_FREE_QUERY_START_GAPS and BA_LOCAL_START;
`full_matrix_profile` is the sequence-to-profile recurrence T / Z / V / H, one profile column at a time. Both return the whole H, so
`own_mode` reads BA_EXACT_GLOBAL (with the last-row rule of BA_FREE_QUERY_END_GAPS) and BA_EXACT_EXTEND off it with `exact_dp.extend_of`.
The two `*_cells` functions state the same recurrences one cell at a time, with nothing folded into a prefix maximum: slow, for the CPU
tests that pin the vectorised forms on small inputs."""
from __future__ import annotations

import numpy as np

from block_aligner_amd.verify import _upper
from tests.exact_dp import NEG, _table, extend_of


def _bytes_of(q: bytes, r: bytes, matrix):
    qa = np.frombuffer(q, np.uint8).astype(np.int64)
    ra = np.frombuffer(r, np.uint8).astype(np.int64)
    if getattr(matrix, "KIND", 1) != 2:
        qa, ra = _upper(qa), _upper(ra)
    return qa, ra


def full_matrix_mode(q: bytes, r: bytes, matrix, gaps, local_start: bool = False, free_query_start: bool = False) -> np.ndarray:
    """H[0 .. |q|][0 .. |r|] (int64). free_query_start: H[0][j] = 0 for every j. local_start: H[0][j] = H[i][0] = 0 and
    H[i][j] = max(0, diagonal, V, Z). Needs open <= extend: a horizontal gap then never opens from a cell that a horizontal gap reached, so
    Z is a prefix maximum over the row without its horizontal gaps (floored first, under local_start)."""
    tab = _table(matrix)
    qa, ra = _bytes_of(q, r, matrix)
    nq, nr = len(qa), len(ra)
    o, e = int(gaps[0]), int(gaps[1])
    assert o <= e < 0
    j = np.arange(nr + 1, dtype=np.int64)
    H = np.empty((nq + 1, nr + 1), np.int64)
    H[0, 0] = 0
    H[0, 1:] = 0 if (local_start or free_query_start) else o + (j[1:] - 1) * e
    V = np.full(nr + 1, NEG, np.int64)
    for i in range(1, nq + 1):
        V = np.maximum(V + e, H[i - 1] + o)
        T = np.empty(nr + 1, np.int64)
        T[0] = 0 if local_start else o + (i - 1) * e
        if nr:
            T[1:] = np.maximum(H[i - 1, :-1] + tab[qa[i - 1], ra], V[1:])
        if local_start:
            T = np.maximum(T, 0)
        pm = np.maximum.accumulate(T - j * e)
        H[i] = T
        if nr:
            H[i, 1:] = np.maximum(T[1:], pm[:-1] + o + (j[1:] - 1) * e)
        V[0] = NEG
    return H


def full_matrix_mode_cells(q: bytes, r: bytes, matrix, gaps, local_start: bool = False, free_query_start: bool = False) -> np.ndarray:
    """full_matrix_mode, one cell at a time: H, V and Z exactly as the header writes them."""
    tab = _table(matrix)
    qa, ra = _bytes_of(q, r, matrix)
    nq, nr = len(qa), len(ra)
    o, e = int(gaps[0]), int(gaps[1])
    H = [[0] * (nr + 1) for _ in range(nq + 1)]
    V = [[NEG] * (nr + 1) for _ in range(nq + 1)]
    for c in range(1, nr + 1):
        H[0][c] = 0 if (local_start or free_query_start) else o + (c - 1) * e
    for i in range(1, nq + 1):
        H[i][0] = 0 if local_start else o + (i - 1) * e
        Z = NEG
        for c in range(1, nr + 1):
            V[i][c] = max(H[i - 1][c] + o, V[i - 1][c] + e)
            Z = max(H[i][c - 1] + o, Z + e)
            h = max(H[i - 1][c - 1] + int(tab[qa[i - 1], ra[c - 1]]), V[i][c], Z)
            H[i][c] = max(h, 0) if local_start else h
    return np.array(H, np.int64).reshape(nq + 1, nr + 1)


def _profile_arrays(q: bytes, profile):
    qa = _upper(np.frombuffer(q, np.uint8)).astype(np.int64) - 65
    sc = profile.pos_aa.astype(np.int64)                                  # [position][residue]
    oC, cC, oR = (np.asarray(x, np.int64) for x in (profile.pos_gap_open_C, profile.pos_gap_close_C, profile.pos_gap_open_R))
    return qa, sc, oC, cC, oR, int(profile.gap_extend)


def full_matrix_profile(q: bytes, profile) -> np.ndarray:
    """H[0 .. |q|][0 .. len(profile)] (int64) of the header's profile recurrence: Z (a run of profile positions against no residue) opens
    from H at open_C[j] + extend and closes into T at close_C[j]; V (a run of residues after position j) opens from T at open_R[j] + extend,
    so inside a column it is a prefix maximum over T; H = max(T, V). Positions that were never set hold -128 and are taken as they are."""
    qa, sc, oC, cC, oR, e = _profile_arrays(q, profile)
    nq, nr = len(qa), profile.str_len
    i = np.arange(nq + 1, dtype=np.int64)
    H = np.empty((nq + 1, nr + 1), np.int64)
    H[0, 0] = 0
    H[1:, 0] = oR[0] + i[1:] * e                                          # T[0][0] = 0 is the only cell V can open from in column 0
    Z = np.full(nq + 1, NEG, np.int64)
    for j in range(1, nr + 1):
        Z = np.maximum(H[:, j - 1] + oC[j] + e, Z + e)
        T = Z + cC[j]
        if nq:
            T[1:] = np.maximum(T[1:], H[:-1, j - 1] + sc[j, qa])
        pm = np.maximum.accumulate(T - i * e)
        H[:, j] = T
        if nq:
            H[1:, j] = np.maximum(T[1:], pm[:-1] + oR[j] + i[1:] * e)
    return H


def full_matrix_profile_cells(q: bytes, profile) -> np.ndarray:
    """full_matrix_profile, one cell at a time: T, Z, V and H exactly as the header writes them."""
    qa, sc, oC, cC, oR, e = _profile_arrays(q, profile)
    nq, nr = len(qa), profile.str_len
    sc, oC, cC, oR, qa = sc.tolist(), oC.tolist(), cC.tolist(), oR.tolist(), qa.tolist()
    H, T, Z, V = ([[NEG] * (nr + 1) for _ in range(nq + 1)] for _ in range(4))
    for i in range(nq + 1):
        for j in range(nr + 1):
            if j >= 1:
                Z[i][j] = max(H[i][j - 1] + oC[j] + e, Z[i][j - 1] + e)
            if i >= 1:
                V[i][j] = max(T[i - 1][j] + oR[j] + e, V[i - 1][j] + e)
            t = 0 if i == 0 and j == 0 else NEG
            if i >= 1 and j >= 1:
                t = max(t, H[i - 1][j - 1] + sc[j][qa[i - 1]])
            if j >= 1:
                t = max(t, Z[i][j] + cC[j])
            T[i][j] = t
            H[i][j] = max(t, V[i][j])
    return np.array(H, np.int64).reshape(nq + 1, nr + 1)


def own_mode(H: np.ndarray, what: str, x_drop: int = -1, free_query_end: bool = False):
    """The record (score, i, j, rows) of BA_EXACT_GLOBAL | BA_EXACT_OWN_MODE ("global") or BA_EXACT_EXTEND | BA_EXACT_OWN_MODE ("extend")
    over a full matrix. free_query_end: GLOBAL reads the maximum of the last row, ties to the smallest j, with no floor at 0."""
    nq, nr = H.shape[0] - 1, H.shape[1] - 1
    if what == "extend":
        return extend_of(H, x_drop)
    if free_query_end:
        j = int(np.argmax(H[nq]))
        return int(H[nq, j]), nq, j, nq + 1
    return int(H[nq, nr]), nq, nr, nq + 1
