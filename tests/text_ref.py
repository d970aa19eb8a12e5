"""Alignment strings in pure Python: the reference the device's ba_*_text output is compared with (tests/test_gpu_text.py, tools/text_rate.py).

An alignment is its CIGAR runs (op | len << 4, ops 1..5 = M = X I D) in alignment order from its first cell (q_start, r_start). M / = / X
columns consume q[i] and r[j], I consumes q[i], D consumes r[j]. The letters are the batch's image letters (image_letters): uppercase for
NucMatrix, 'A' + code (the uppercased letter) for AAMatrix, the raw bytes for ByteMatrix, and the reverse complement of the caller's query for
a minus-strand seed."""
import re

OP_CHARS = " M=XID"
MD_RE = re.compile(r"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
CIGAR, MD, CS = 0, 1, 2
FAILED = 1 | 2 | 4 | 8 | 16 | 32 | 128   # overflow, lost and watchdog status bits: empty text
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def kind_of(matrix) -> str:
    """'aa', 'nuc' or 'bytes' for a scores.* matrix (its KIND: 0, 1, 2)."""
    return ("aa", "nuc", "bytes")[getattr(matrix, "KIND", 1)]


def image_letters(seq: bytes, kind: str = "nuc", minus: bool = False) -> bytes:
    """The letters of a sequence's image: uppercase ASCII except for ByteMatrix batches; minus: reverse complement (A<->T, C<->G)."""
    seq = bytes(seq)
    if kind == "bytes":
        return seq
    up = seq.upper()
    return up[::-1].translate(_COMP) if minus else up


def consumed(runs):
    """(query, reference) cells the runs consume."""
    cq = cr = 0
    for x in runs:
        op, n = int(x) & 15, int(x) >> 4
        cq += n if op in (1, 2, 3, 4) else 0
        cr += n if op in (1, 2, 3, 5) else 0
    return cq, cr


def cigar(runs, q_start: int = 0, q_len: int = 0, soft_clip: bool = False) -> str:
    """<len><op> per run; soft_clip: <q_start>S in front when q_start > 0, <q_len - q_end>S behind when that is > 0."""
    runs = [int(x) for x in runs]
    if not runs:
        return ""
    s = "".join(f"{x >> 4}{OP_CHARS[x & 15]}" for x in runs)
    if soft_clip:
        q_end = q_start + consumed(runs)[0]
        s = (f"{q_start}S" if q_start > 0 else "") + s + (f"{q_len - q_end}S" if q_len > q_end else "")
    return s


def md(runs, q: bytes, r: bytes, q_start: int, r_start: int) -> str:
    """SAM MD:Z value: equal match-type columns count; a mismatch emits the count and the reference letter, a D run the count, '^' and its
    letters; I columns emit nothing; the count closes the string."""
    runs = [int(x) for x in runs]
    if not runs:
        return ""
    i, j, n, out = q_start, r_start, 0, []
    for x in runs:
        op, ln = x & 15, x >> 4
        if op in (1, 2, 3):
            for k in range(ln):
                if q[i + k] == r[j + k]:
                    n += 1
                else:
                    out.append(f"{n}{chr(r[j + k])}")
                    n = 0
            i += ln
            j += ln
        elif op == 4:
            i += ln
        elif op == 5:
            out.append(f"{n}^{r[j:j + ln].decode('latin-1')}")
            n = 0
            j += ln
    out.append(str(n))
    return "".join(out)


def cs(runs, q: bytes, r: bytes, q_start: int, r_start: int) -> str:
    """minimap2's short cs:Z value: :<n> per stretch of equal columns, *<ref><query> per mismatch, +<query> per I run, -<ref> per D run,
    letters lowercase."""
    runs = [int(x) for x in runs]
    if not runs:
        return ""
    i, j, n, out = q_start, r_start, 0, []

    def flush():
        nonlocal n
        if n:
            out.append(f":{n}")
        n = 0

    for x in runs:
        op, ln = x & 15, x >> 4
        if op in (1, 2, 3):
            for k in range(ln):
                if q[i + k] == r[j + k]:
                    n += 1
                else:
                    flush()
                    out.append("*" + bytes([r[j + k], q[i + k]]).lower().decode("latin-1"))
            i += ln
            j += ln
        elif op == 4:
            flush()
            out.append("+" + q[i:i + ln].lower().decode("latin-1"))
            i += ln
        elif op == 5:
            flush()
            out.append("-" + r[j:j + ln].lower().decode("latin-1"))
            j += ln
    flush()
    return "".join(out)


def render(what: int, runs, q: bytes, r: bytes, q_start: int, r_start: int, soft_clip: bool = False, status: int = 0) -> str:
    """One pair's text as ba_*_text renders it; q and r are image letters (image_letters), q the whole query (its length is the soft clips')."""
    if status & FAILED:
        return ""
    if what == CIGAR:
        return cigar(runs, q_start, len(q), soft_clip)
    return (md if what == MD else cs)(runs, q, r, q_start, r_start)


def md_parts(s: str):
    """(equal columns, mismatch letters, deleted letters) of an MD value."""
    assert MD_RE.fullmatch(s), s
    eq = sum(int(x) for x in re.findall(r"[0-9]+", s))
    dels = sum(len(x) - 1 for x in re.findall(r"\^[A-Z]+", s))
    letters = sum(1 for c in s if c.isalpha())
    return eq, letters - dels, dels


def cs_replay(s: str, r_seg: bytes):
    """Replay a cs value along r_seg (the reference from r_start, uppercase): -> (query segment, reference segment), uppercase."""
    qo, ro, j = [], [], 0
    for tok in re.findall(r":[0-9]+|\*[a-z][a-z]|\+[a-z]+|-[a-z]+|.", s):
        if tok[0] == ":":
            n = int(tok[1:])
            qo.append(r_seg[j:j + n]); ro.append(r_seg[j:j + n]); j += n
        elif tok[0] == "*":
            ro.append(tok[1].upper().encode()); qo.append(tok[2].upper().encode()); j += 1
        elif tok[0] == "+":
            qo.append(tok[1:].upper().encode())
        elif tok[0] == "-":
            ro.append(tok[1:].upper().encode()); j += len(tok) - 1
        else:
            raise AssertionError(f"bad cs token {tok!r} in {s!r}")
    return b"".join(qo), b"".join(ro)
