"""The Python reference of the alignment strings (tests/text_ref.py), pinned on hand-made alignments: the worked example of INTEGRATION.md,
the MD corner cases, cs's stretch rule, soft clips, the image letters -- and the SAM grammar of every MD it renders."""
import numpy as np

from tests import text_ref as T


def runs(s: str):
    """'4M1D3M' -> packed runs"""
    out, n = [], ""
    for c in s:
        if c.isdigit():
            n += c
        else:
            out.append(int(n) << 4 | T.OP_CHARS.index(c))
            n = ""
    return out


Q, R = b"ACCTAGTTTAC", b"ACGTACGTAC"
EX = runs("4M1D3M2I2M")


def test_worked_example():
    assert T.render(T.CIGAR, EX, Q, R, 0, 0) == "4M1D3M2I2M"
    assert T.render(T.MD, EX, Q, R, 0, 0) == "2G1^A0C4"
    assert T.render(T.CS, EX, Q, R, 0, 0) == ":2*gc:1-a*ca:2+tt:2"


def test_worked_example_with_cigar_eq():
    eq = runs("2=1X1=1D1X2=2I2=")
    assert T.render(T.CIGAR, eq, Q, R, 0, 0) == "2=1X1=1D1X2=2I2="
    assert T.render(T.MD, eq, Q, R, 0, 0) == "2G1^A0C4"
    assert T.render(T.CS, eq, Q, R, 0, 0) == ":2*gc:1-a*ca:2+tt:2"


def test_mismatch_right_after_a_deletion():
    assert T.md(runs("1M2D2M"), b"AGG", b"AACTG", 0, 0) == "1^AC0T1"
    assert T.cs(runs("1M2D2M"), b"AGG", b"AACTG", 0, 0) == ":1-ac*tg:1"


def test_adjacent_mismatches():
    assert T.md(runs("4M"), b"AGTA", b"ACGA", 0, 0) == "1C0G1"
    assert T.md(runs("2M"), b"TT", b"AC", 0, 0) == "0A0C0"
    assert T.cs(runs("2M"), b"TT", b"AC", 0, 0) == "*at*ct"


def test_insertion_between_equal_stretches():
    q, r, x = b"ACTTGT", b"ACGT", runs("2M2I2M")
    assert T.md(x, q, r, 0, 0) == "4"   # MD: I does not break the count
    assert T.cs(x, q, r, 0, 0) == ":2+tt:2"   # cs: it ends the stretch


def test_insertion_only_and_empty_alignments():
    assert T.md(runs("3I"), b"ACG", b"", 0, 0) == "0"
    assert T.cs(runs("3I"), b"ACG", b"", 0, 0) == "+acg"
    assert T.cigar(runs("3I")) == "3I"
    for w in (T.CIGAR, T.MD, T.CS):
        assert T.render(w, [], b"ACGT", b"ACGT", 2, 2) == ""
        assert T.render(w, EX, Q, R, 0, 0, status=4) == ""   # a failure bit: no text


def test_soft_clips_on_both_ends():
    q = b"GG" + Q + b"TTT"
    assert T.cigar(EX, 2, len(q), True) == "2S4M1D3M2I2M3S"
    assert T.cigar(EX, 2, len(q), False) == "4M1D3M2I2M"
    assert T.cigar(EX, 0, len(Q), True) == "4M1D3M2I2M"
    assert T.render(T.CIGAR, EX, q, R, 2, 0, soft_clip=True) == "2S4M1D3M2I2M3S"
    assert T.render(T.MD, EX, q, R, 2, 0) == "2G1^A0C4"


def test_image_letters():
    assert T.image_letters(b"acgtN", "nuc") == b"ACGTN"
    assert T.image_letters(b"aacG", "nuc", minus=True) == b"CGTT"
    assert T.image_letters(b"wRk", "aa") == b"WRK"
    assert T.image_letters(b"aA", "bytes") == b"aA"


def test_md_and_cs_cross_checks_on_random_alignments():
    """Random paths over random sequences: every MD matches the SAM grammar, its counts and letters add up to the reference consumed, its
    edits plus the CIGAR's I are the edit distance, and replaying cs rebuilds both segments."""
    rng = np.random.default_rng(7)
    for _ in range(400):
        ops = []
        for _ in range(int(rng.integers(1, 12))):
            op = int(rng.choice([1, 1, 1, 2, 3, 4, 5]))
            n = int(rng.integers(1, 9))
            if ops and ops[-1][0] == op:
                ops[-1][1] += n
            else:
                ops.append([op, n])
        x = [n << 4 | op for op, n in ops]
        cq, cr = T.consumed(x)
        q0, r0 = int(rng.integers(0, 5)), int(rng.integers(0, 5))
        q = bytes(rng.choice(list(b"ACGT"), q0 + cq + 3).astype(np.uint8))
        r = bytes(rng.choice(list(b"ACGT"), r0 + cr + 2).astype(np.uint8))
        m = T.md(x, q, r, q0, r0)
        assert T.MD_RE.fullmatch(m), m
        eq, mis, dels = T.md_parts(m)
        assert eq + mis + dels == cr
        ins = sum(n for op, n in ops if op == 4)
        edits = sum(1 for op, n in ops if op in (1, 2, 3) for k in range(n)) - eq + ins + dels
        assert mis + dels + ins == edits
        c = T.cs(x, q, r, q0, r0)
        assert T.cs_replay(c, r[r0:]) == (q[q0:q0 + cq], r[r0:r0 + cr]), (c, ops)
        assert T.cigar(x, q0, len(q), True).startswith(f"{q0}S" if q0 else str(ops[0][1]))
