"""Full-matrix affine-gap DP of small pairs, in numpy (test infrastructure; own code, written from the definitions in
include/block_aligner_hip.h, "exact full-matrix scores"; no oracle/ and no reference code).

`full_matrix` keeps every row of H, built row by row in the manner of tests/gotoh.py (whose `global_score` its corner must equal);
`exact_global` and `exact_extend` read the two quantities of the ba_*_exact calls off it."""
from __future__ import annotations

import numpy as np

from block_aligner_amd.verify import _upper, score_table

NEG = -(1 << 40)
_tables = {}


def _table(matrix) -> np.ndarray:
    """score_table(matrix), built once per matrix object (the object is kept, so its id stays its own)."""
    ent = _tables.get(id(matrix))
    if ent is None:
        ent = _tables[id(matrix)] = (matrix, score_table(matrix))
    return ent[1]


def full_matrix(q: bytes, r: bytes, matrix, gaps) -> np.ndarray:
    """H[0 .. |q|][0 .. |r|] (int64): H[0][0] = 0, a gap of length n costs open + (n - 1) extend. NucMatrix / AAMatrix score the uppercased
    bytes (what the images hold), ByteMatrix the raw bytes."""
    tab = _table(matrix)
    qa = np.frombuffer(q, np.uint8).astype(np.int64)
    ra = np.frombuffer(r, np.uint8).astype(np.int64)
    if getattr(matrix, "KIND", 1) != 2:
        qa, ra = _upper(qa), _upper(ra)
    nq, nr = len(qa), len(ra)
    o, e = int(gaps[0]), int(gaps[1])
    j = np.arange(nr + 1, dtype=np.int64)
    H = np.empty((nq + 1, nr + 1), np.int64)
    H[0, 0] = 0
    H[0, 1:] = o + (j[1:] - 1) * e
    V = np.full(nr + 1, NEG, np.int64)               # best score ending in a gap that consumes query only
    for i in range(1, nq + 1):
        V = np.maximum(V + e, H[i - 1] + o)
        T = np.empty(nr + 1, np.int64)               # the row without its horizontal gaps
        T[0] = o + (i - 1) * e
        if nr:
            T[1:] = np.maximum(H[i - 1, :-1] + tab[qa[i - 1], ra], V[1:])
        # a horizontal gap into column j opens at the best T[k], k < j: T[k] + o + (j - k - 1) e
        pm = np.maximum.accumulate(T - j * e)
        H[i] = T
        if nr:
            H[i, 1:] = np.maximum(T[1:], pm[:-1] + o + (j[1:] - 1) * e)
        V[0] = NEG
    return H


def exact_global(q: bytes, r: bytes, matrix, gaps):
    """BA_EXACT_GLOBAL -> (score, i, j, rows)."""
    H = full_matrix(q, r, matrix, gaps)
    return int(H[len(q), len(r)]), len(q), len(r), len(q) + 1


def extend_of(H: np.ndarray, x_drop: int = -1):
    """BA_EXACT_EXTEND over a full matrix -> (score, i, j, rows). x_drop < 0: the maximum over every cell. x_drop >= 0: rows in order;
    after row i, if its maximum is below (the largest row maximum so far, row i included) - x_drop, the later rows do not count. Ties: the
    smallest i, then the smallest j."""
    best, bi, bj = None, 0, 0
    rows = H.shape[0]
    for i in range(H.shape[0]):
        jm = int(np.argmax(H[i]))                   # (the first maximum of the row)
        rm = int(H[i, jm])
        if best is None or rm > best:
            best, bi, bj = rm, i, jm
        if x_drop >= 0 and rm < best - x_drop:
            rows = i + 1
            break
    return int(best), bi, bj, rows


def exact_extend(q: bytes, r: bytes, matrix, gaps, x_drop: int = -1):
    return extend_of(full_matrix(q, r, matrix, gaps), x_drop)
