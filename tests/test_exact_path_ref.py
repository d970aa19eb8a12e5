"""The tests' own path helper (tests/exact_path.py) without a GPU: its H is the full matrix of tests/exact_dp.py, its runs are a path from
(0, 0) to the exact end cell that rescores to the exact score (verify.check_cigar), and a hand-worked tie case gives the runs the rule
prescribes."""
import numpy as np
import pytest

from block_aligner_amd import scores as S
from block_aligner_amd.verify import check_cigar
from tests import exact_dp, exact_path

OPS = {1: "M", 2: "=", 3: "X", 4: "I", 5: "D"}


def text(runs):
    return "".join(f"{int(x) >> 4}{OPS[int(x) & 15]}" for x in runs)


def cases(kind):
    rng = np.random.default_rng({"nuc": 21, "aa": 22, "bytes": 23}[kind])
    if kind == "nuc":
        m, gaps, alphabet = S.NucMatrix.new_simple(2, -3), (-5, -1), np.frombuffer(b"ACGT", np.uint8)
    elif kind == "aa":
        m, gaps, alphabet = S.static_matrix("BLOSUM62"), (-11, -1), np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    else:
        m, gaps, alphabet = S.ByteMatrix.new_simple(3, -2), (-4, -2), np.arange(250, 256, dtype=np.uint8)
    pairs = []
    for nq, nr in [(0, 0), (0, 5), (7, 0), (1, 1), (129, 129), (129, 3), (2, 128)] + [tuple(int(x) for x in rng.integers(0, 130, 2)) for _ in range(25)]:
        base = alphabet[rng.integers(0, len(alphabet), max(nq, nr) + 8)]
        q = base[:nq].copy()
        if nq > 10:                                   # an edit and an indel, so that gaps are on the path
            q[int(rng.integers(0, nq))] = alphabet[0]
            k = int(rng.integers(1, nq - 5))
            q = np.concatenate([q[:k], q[k + 4:], alphabet[rng.integers(0, len(alphabet), 4)]])
        qb, rb = q.tobytes(), base[:nr].tobytes()
        pairs.append((qb.lower(), rb) if kind != "bytes" and len(pairs) % 3 == 0 else (qb, rb))
    return m, gaps, pairs


@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_helper_matrix_and_paths(kind):
    m, gaps, pairs = cases(kind)
    assert max(len(q) for q, _ in pairs) == 129 and min(len(q) for q, _ in pairs) == 0
    gapped = 0
    for q, r in pairs:
        H, V, Z = exact_path.matrices(q, r, m, gaps)
        assert np.array_equal(H, exact_dp.full_matrix(q, r, m, gaps)), (q, r)
        for what, x, eq in (("global", -1, False), ("global", -1, True), ("extend", -1, True), ("extend", 0, False), ("extend", 30, True)):
            rec, runs = exact_path.exact_runs(q, r, m, gaps, what, x, eq)
            want = exact_dp.exact_global(q, r, m, gaps) if what == "global" else exact_dp.exact_extend(q, r, m, gaps, x)
            assert rec == want
            qa, ra = exact_path.images(q, r, m)
            check_cigar(runs, bytes(qa.astype(np.uint8)), bytes(ra.astype(np.uint8)), m, gaps, rec[0], rec[1], rec[2], what=(q, r, what, x))
            ops = {int(x) & 15 for x in runs}
            assert ops <= ({2, 3, 4, 5} if eq else {1, 4, 5})
            gapped += bool(ops & {4, 5}) and bool(ops & {1, 2, 3})
            if rec[0] == 0 and rec[1] == 0 and rec[2] == 0:
                assert runs == []
    assert gapped > 20


def test_hand_worked_ties():
    """q = AAAAA against r = AAAA, match 2, mismatch -3, gaps (-5, -1): one query letter is inserted, and every position of the insertion
    gives the same score 4 * 2 - 5 = 3. From (5, 4) the diagonal is optimal (H[4][3] = 3 * 2 - 5 = 1, 1 + 2 = 3 = H[5][4]) and stays so
    down to (1, 0), so the walk takes the four matches first and the insertion is the alignment's first column."""
    m, gaps = S.NucMatrix.new_simple(2, -3), (-5, -1)
    rec, runs = exact_path.exact_runs(b"AAAAA", b"AAAA", m, gaps)
    assert rec == (3, 5, 4, 6) and text(runs) == "1I4M"
    rec, runs = exact_path.exact_runs(b"AAAA", b"AAAAA", m, gaps)
    assert rec == (3, 4, 5, 5) and text(runs) == "1D4M"
    # two letters too many: one gap of two (2 * 4 - 5 - 1 = 2), never two gaps of one (8 - 10); extension is preferred inside it
    rec, runs = exact_path.exact_runs(b"AAAAAA", b"AAAA", m, gaps)
    assert rec == (2, 6, 4, 7) and text(runs) == "2I4M"
    # the inserted letter is marked: q = AATAA. The diagonal wins wherever it ties, so the walk takes AA, then the I, then AA
    rec, runs = exact_path.exact_runs(b"AATAA", b"AAAA", m, gaps, eq=True)
    assert rec == (3, 5, 4, 6) and text(runs) == "2=1I2="
    # linear gaps (open == extend): a gap of two costs -2, merged into one run although each column "opens"
    rec, runs = exact_path.exact_runs(b"AAAAAA", b"AAAA", m, (-1, -1))
    assert rec == (6, 6, 4, 7) and text(runs) == "2I4M"
    # EXTEND ends at the first maximum: AAAA / AAAA then junk
    rec, runs = exact_path.exact_runs(b"AAAACCCC", b"AAAAGGGG", m, gaps, "extend", -1, True)
    assert rec == (8, 4, 4, 9) and text(runs) == "4="
    # nothing aligns: score 0 at (0, 0), no runs
    rec, runs = exact_path.exact_runs(b"CCCC", b"GGGG", m, gaps, "extend", 0)
    assert rec[:3] == (0, 0, 0) and runs == []
