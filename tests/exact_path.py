"""Optimal alignment paths of the full-matrix affine-gap DP, in numpy / Python (test infrastructure; own code, written from the definition
in include/block_aligner_hip.h, "optimal alignment paths"; no oracle/ and no reference code).

`matrices` keeps every row of H, V (best score ending in a gap that consumes the query, CIGAR I) and Z (... the reference, D); `walk` goes
backwards from an end cell by the rule and returns the merged runs in alignment order, packed as the library packs them
(length << 4 | op; op 1 M, 2 =, 3 X, 4 I, 5 D); `exact_runs` does both for the end cell of a ba_*_exact record."""
from __future__ import annotations

import numpy as np

from block_aligner_amd.verify import _upper, score_table
from tests import exact_dp

NEG = -(1 << 40)     # "no cell": V and Z in row 0 and column 0
_tables = {}
_cache = {}


def _table(matrix) -> np.ndarray:
    ent = _tables.get(id(matrix))
    if ent is None:
        ent = _tables[id(matrix)] = (matrix, score_table(matrix))
    return ent[1]


def images(q: bytes, r: bytes, matrix):
    """What the device's sequence images hold, as far as scores and '=' / 'X' go: uppercased bytes for NucMatrix / AAMatrix, raw for ByteMatrix."""
    qa = np.frombuffer(q, np.uint8).astype(np.int64)
    ra = np.frombuffer(r, np.uint8).astype(np.int64)
    if getattr(matrix, "KIND", 1) != 2:
        qa, ra = _upper(qa), _upper(ra)
    return qa, ra


def matrices(q: bytes, r: bytes, matrix, gaps):
    """-> (H, V, Z), int64 arrays of (|q| + 1, |r| + 1). For i, j >= 1: V[i][j] = max(H[i-1][j] + open, V[i-1][j] + extend),
    Z[i][j] = max(H[i][j-1] + open, Z[i][j-1] + extend), H[i][j] = max(H[i-1][j-1] + s, V[i][j], Z[i][j]); the borders of H are pure gaps."""
    tab = _table(matrix)
    qa, ra = images(q, r, matrix)
    nq, nr = len(qa), len(ra)
    o, e = int(gaps[0]), int(gaps[1])
    H = np.empty((nq + 1, nr + 1), np.int64)
    V = np.full((nq + 1, nr + 1), NEG, np.int64)
    Z = np.full((nq + 1, nr + 1), NEG, np.int64)
    H[0, 0] = 0
    for j in range(1, nr + 1):
        H[0, j] = o + (j - 1) * e
    jj = np.arange(nr + 1, dtype=np.int64)
    for i in range(1, nq + 1):
        H[i, 0] = o + (i - 1) * e
        if nr:
            V[i, 1:] = np.maximum(H[i - 1, 1:] + o, V[i - 1, 1:] + e)
            T = np.empty(nr + 1, np.int64)           # the row without its horizontal gaps
            T[0] = H[i, 0]
            T[1:] = np.maximum(H[i - 1, :-1] + tab[qa[i - 1], ra], V[i, 1:])
            # a horizontal gap into column j opens at the best T[k], k < j (opening at a cell that is itself a gap's end never beats
            # extending that gap, open <= extend): Z[i][j] = max over k < j of T[k] + open + (j - k - 1) extend
            Z[i, 1:] = np.maximum.accumulate(T - jj * e)[:-1] + o + (jj[1:] - 1) * e
            H[i, 1:] = np.maximum(T[1:], Z[i, 1:])
            # ... which is the recurrence as it is written, cell by cell
            assert (Z[i, 1:] == np.maximum(H[i, :-1] + o, Z[i, :-1] + e)).all()
    return H, V, Z


def walk(H, V, Z, qa, ra, tab, gaps, i: int, j: int, eq: bool = False):
    """The path's runs, from the end cell (i, j) backwards to (0, 0) by the rule, returned in alignment order and merged."""
    e = int(gaps[1])
    ops = []                                         # reversed, one per column
    state = "H"
    while True:
        if state == "H":
            if i == 0:
                ops += [5] * j
                break
            if j == 0:
                ops += [4] * i
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
            state = "V" if V[i, j] == V[i - 1, j] + e else "H"       # extension is preferred
            i -= 1
        else:
            ops.append(5)
            state = "Z" if Z[i, j] == Z[i, j - 1] + e else "H"
            j -= 1
    runs = []
    for op in reversed(ops):
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    return [(n << 4) | op for op, n in runs]


def exact_runs(q: bytes, r: bytes, matrix, gaps, what: str = "global", x_drop: int = -1, eq: bool = False):
    """-> ((score, i, j, rows), runs) of BA_EXACT_GLOBAL ("global") or BA_EXACT_EXTEND ("extend", with x_drop). The matrices of a pair are
    computed once and kept."""
    key = (q, r, id(matrix), tuple(gaps))
    ent = _cache.get(key)
    if ent is None:
        ent = _cache[key] = (matrix, matrices(q, r, matrix, gaps))
    H, V, Z = ent[1]
    rec = (int(H[len(q), len(r)]), len(q), len(r), len(q) + 1) if what == "global" else exact_dp.extend_of(H, x_drop)
    qa, ra = images(q, r, matrix)
    return rec, walk(H, V, Z, qa, ra, _table(matrix), gaps, rec[1], rec[2], eq)
