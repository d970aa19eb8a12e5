"""A model of seeding both strands of a read at once ("Both strands at once"), in integers: the sketch over canonical
k-mers, the entries of a canonical index over several sequences, and the hits of a read on both strands -- problem 2 r + s is read r on
strand s. The rule is written twice, as in tests/seeding_ref.py: sketch_plain() / entries_plain() / hits_plain() spell it out position by
position in plain Python; sketch() / entries() / hits() are the same in NumPy on top of tests/seeding_ref.py and tests/index_multi_ref.py.
hits() is what Seeder.indexed_both must report for one read, bit for bit. The plain functions also take one of MISTAKES, a neighbouring
rule that an implementation could follow instead: every case the GPU tests use must tell the rule from them. Also the case builders that
the CPU and the GPU tests share."""
from collections import namedtuple

import numpy as np

from tests import index_multi_ref as M, index_ref as X, seeding_ref as S

Params = X.Params   # k w max_occ max_ref_occ
NO_CAP = S.NO_CAP
STRAND_BIT = 1 << 31
POS_MASK = STRAND_BIT - 1
MISTAKES = ("strand_in_order_key", "caps_per_strand", "minus_q_off_by_k", "palindrome_kept")

Read = namedtuple("Read", "pos code strand")


def revcomp(s: bytes) -> bytes:
    return S.oriented(bytes(s), 1)


# ------------------------------------------------------------------ the rule, position by position
def canon_plain(seq: bytes, k: int, mistake=None):
    """-> per k-mer (canonical code, strand bit), None for an invalid one: a byte outside ACGT, or a palindrome."""
    out = []
    for i, f in enumerate(S.codes_plain(seq, k)):
        if f is None:
            out.append(None)
            continue
        g = 0
        for t in range(k):
            g |= (3 - S._CODE[seq[i + t]]) << (2 * t)
        if f == g and mistake != "palindrome_kept":
            out.append(None)
        else:
            out.append((min(f, g), 1 if g < f else 0))
    return out


def sketch_plain(seq: bytes, k: int, w: int, mistake=None):
    """-> [(pos, code, strand)] of the selected k-mers, ascending by position. The smallest h(code) of a window wins, the leftmost of equals."""
    cs = canon_plain(bytes(seq), k, mistake)
    nk = len(cs)
    if nk == 0:
        return []
    windows = [(0, nk)] if nk <= w else [(a, a + w) for a in range(nk - w + 1)]
    order = (lambda i: (S.h32(cs[i][0]), cs[i][1], i)) if mistake == "strand_in_order_key" else (lambda i: (S.h32(cs[i][0]), i))
    sel = set()
    for a, b in windows:
        best = None
        for i in range(a, b):
            if cs[i] is not None and (best is None or order(i) < order(best)):
                best = i
        if best is not None:
            sel.add(best)
    return [(i, cs[i][0], cs[i][1]) for i in sorted(sel)]


def entries_plain(seqs, k: int, w: int, mistake=None):
    """-> [(code, strand, pos)] of the index, ascending, positions in the index's frame: every sequence's own sketch, shifted by its start."""
    out = []
    for s, at in zip(seqs, M.seq_start(seqs)):
        out += [(c, st, at + i) for i, c, st in sketch_plain(s, k, w, mistake)]
    return sorted(out)


def hits_plain(read: bytes, seqs, P: Params, mistake=None):
    """-> ([(q_hit, r_hit)] of the plus problem, the same of the minus problem), each in the order of the rule, (r_hit, q_hit)."""
    index = entries_plain(seqs, P.k, P.w, mistake)
    sk = sketch_plain(read, P.k, P.w, mistake)
    n = len(read)
    out = ([], [])
    per = mistake == "caps_per_strand"   # (the mistake: a code's entries are counted on each strand apart)
    in_read, in_index, at = {}, {}, {}
    for _, c, sq in sk:
        in_read[(c, sq if per else 0)] = in_read.get((c, sq if per else 0), 0) + 1
    for c, sr, j in index:
        in_index[(c, sr if per else 0)] = in_index.get((c, sr if per else 0), 0) + 1
        at.setdefault(c, []).append((sr, j))
    for i, c, sq in sk:
        mq = in_read[(c, sq if per else 0)]   # the read's entries with this code, both strands together
        for sr, j in at.get(c, []):
            m = in_index[(c, sr if per else 0)]   # the index's
            if mq > P.max_occ or m > P.max_ref_occ:
                continue
            rel = sq ^ sr
            flip = n - 1 - i if mistake == "minus_q_off_by_k" else n - P.k - i
            out[rel].append((flip if rel else i, j))
    return tuple(sorted(h, key=lambda x: (x[1], x[0])) for h in out)


# ------------------------------------------------------------------ the same in NumPy
def sketch(seq: bytes, k: int, w: int) -> Read:
    """-> Read(pos, code, strand) as uint32 arrays, ascending by position."""
    two = S._LUT[np.frombuffer(bytes(seq), np.uint8)]
    nk = len(two) - k + 1
    z = np.zeros(0, np.uint32)
    if nk <= 0:
        return Read(z, z, z)
    f, g, bad = np.zeros(nk, np.uint64), np.zeros(nk, np.uint64), np.zeros(nk, bool)
    for t in range(k):
        x = two[t:t + nk]
        bad |= x > 3
        f = f << np.uint64(2) | (x & 3).astype(np.uint64)
        g |= (3 - (x & 3)).astype(np.uint64) << np.uint64(2 * t)
    bad |= f == g
    code, strand = np.minimum(f, g), (g < f).astype(np.uint32)
    key = S.h32_np(code) << np.uint64(32) | np.arange(nk, dtype=np.uint64)
    key[bad] = np.uint64(0xffffffffffffffff)
    mins = key.min(keepdims=True) if nk <= w else np.lib.stride_tricks.sliding_window_view(key, w).min(axis=1)
    mins = np.unique(mins[mins != np.uint64(0xffffffffffffffff)])
    pos = np.sort((mins & np.uint64(S.MASK)).astype(np.int64))
    return Read(pos.astype(np.uint32), code[pos].astype(np.uint32), strand[pos])


def keys(sk: Read, shift: int = 0):
    return np.sort(sk.code.astype(np.uint64) << np.uint64(32) | sk.strand.astype(np.uint64) << np.uint64(31) | (sk.pos.astype(np.uint64) + np.uint64(shift)))


def index_keys(seqs, k: int, w: int):
    parts = [np.zeros(0, np.uint64)] + [keys(sketch(s, k, w), at) for s, at in zip(seqs, M.seq_start(seqs))]
    return np.sort(np.concatenate(parts))


def entries(seqs, k: int, w: int):
    """-> (code, pos with the strand in bit 31) of the index, ascending, and longest_run: a code's entries of both strands together."""
    key = index_keys(seqs, k, w)
    code = (key >> np.uint64(32)).astype(np.uint32)
    longest = int(np.unique(code, return_counts=True)[1].max()) if len(code) else 0
    return code, (key & np.uint64(S.MASK)).astype(np.uint32), longest


def hits(read: bytes, seqs, P: Params, index=None):
    """-> dict(q_pos: with the strand in bit 31, q_code: the read's sketch in position order; problems: [dict(q_hit, r_hit)] of the plus and
    the minus problem). index: index_keys(seqs, k, w), when the caller has it."""
    rk = index_keys(seqs, P.k, P.w) if index is None else index
    sk = sketch(read, P.k, P.w)
    qk = keys(sk)
    one = np.uint64(1)
    code = qk >> np.uint64(32) << np.uint64(32)
    top = code | np.uint64(S.MASK)   # (no low word is 0xffffffff; code + 1 can leave 64 bits)
    mq = np.searchsorted(qk, top, "left") - np.searchsorted(qk, code, "left")
    lo, hi = np.searchsorted(rk, code, "left"), np.searchsorted(rk, top, "left")
    m = hi - lo
    m[(mq > P.max_occ) | (m > P.max_ref_occ)] = 0
    src = np.repeat(np.arange(len(qk)), m)                                           # the read entry of every hit
    at = np.repeat(lo, m) + (np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m))   # its index entry
    sq, i = (qk[src] >> np.uint64(31)) & one, (qk[src] & np.uint64(POS_MASK)).astype(np.int64)
    sr, j = (rk[at] >> np.uint64(31)) & one, (rk[at] & np.uint64(POS_MASK)).astype(np.int64)
    rel = (sq ^ sr).astype(bool)
    q = np.where(rel, len(read) - P.k - i, i)
    problems = []
    for s in (False, True):
        order = np.argsort(j[rel == s] << 32 | q[rel == s], kind="stable")
        problems.append(dict(q_hit=q[rel == s][order].astype(np.uint32), r_hit=j[rel == s][order].astype(np.uint32)))
    return dict(q_pos=(sk.pos | sk.strand << np.uint32(31)).astype(np.uint32), q_code=sk.code, problems=problems)


def expected(reads, seqs, P: Params):
    """-> [hits(read)] per read, over one index."""
    rk = index_keys(seqs, P.k, P.w)
    return [hits(r, seqs, P, rk) for r in reads]


def per_problem(exps):
    """The 2 n problems of n reads' hits() -> [dict(q_hit, r_hit)]: problem 2 r + s."""
    return [p for e in exps for p in e["problems"]]


class Reads:
    """Reads in the layout ba_seeding_create_indexed_both takes: each once, packed into one pool."""

    def __init__(self, reads):
        self.reads = [bytes(q) for q in reads]
        lens = np.array([len(q) for q in self.reads], np.int64)
        self.pool = np.frombuffer(b"".join(self.reads) + b"#", np.uint8).copy()
        self.q_off = (np.cumsum(lens) - lens).astype(np.uint64)
        self.q_len = lens.astype(np.uint32)

    def __len__(self):
        return len(self.reads)

    def args(self):
        return (self.pool, self.q_off, self.q_len)

    def listed_twice(self):
        """The same reads as 2 n problems of Seeder.indexed: problem 2 r + s is read r on strand s -> index_ref.ReadSet."""
        rs = X.ReadSet([])
        rs.reads = [(q, s) for q in self.reads for s in (0, 1)]
        rs.pool, rs.q_off, rs.q_len = self.pool, np.repeat(self.q_off, 2), np.repeat(self.q_len, 2)
        rs.strand = np.tile(np.array([0, 1], np.uint8), len(self))
        return rs


def is_palindrome(mer: bytes) -> bool:
    return revcomp(mer) == bytes(mer).upper()


def mer(rng, k: int) -> bytes:
    """A random k-mer that is no palindrome."""
    while True:
        x = S.dna(rng, k)
        if not is_palindrome(x):
            return x


# ------------------------------------------------------------------ the index sketch
SEAM_WINDOWS = X.SEAM_WINDOWS                     # 1023, 1024, 1025 and 2049 windows: span seams fall inside
INDEX_KW = ((4, 1), (6, 5), (15, 10), (16, 64))   # even k: palindromes; k = 16: a code fills 32 bits


def inverted_repeats(rng, k: int, w: int, n: int = 40) -> bytes:
    """Stretches x + revcomp(x), most without a spacer: the k-mers across the middle have their reverse complements one, two, three ...
    positions on, so a window holds the same canonical code twice, on either strand first. Where that code is the window's minimum the
    leftmost must win, whatever its strand."""
    out = b""
    for _ in range(n):
        x = S.dna(rng, k + int(rng.integers(0, 3)))
        out += x + S.dna(rng, (0, 0, 0, 1, 2)[int(rng.integers(0, 5))]) + revcomp(x) + S.dna(rng, int(rng.integers(0, 4)))
    return out


def index_cases(k: int, w: int, seed: int = 83):
    """-> {name: [sequences]}."""
    rng = np.random.default_rng(seed + 100 * k + w)
    out = {f"random_{nw}": [S.dna(rng, X.ref_len_for_windows(nw, k, w))] for nw in SEAM_WINDOWS}
    out["acgt_repeats"] = [b"ACGT" * 700]   # at k = 4 every second k-mer (ACGT, GTAC) is a palindrome; across the first seam
    base = S.dna(rng, X.ref_len_for_windows(X.SPAN + 1, k, w))
    other = bytearray(bytes(c + 32 if rng.random() < 0.5 else c for c in base))
    for at in rng.integers(0, len(other), 12):
        other[int(at)] = b"NnRy-*"[int(at) % 6]
    run = k + w + 9
    other[X.SPAN - run // 2:X.SPAN - run // 2 + run] = b"N" * run   # whole windows without a k-mer across the seam
    out["lower_case_and_other_bytes"] = [bytes(other)]
    out["inverted_repeats"] = [inverted_repeats(rng, k, w, 150) + S.dna(rng, 300)]
    # four sequences: x straddles the first junction and poly-A the third, revcomp(x) lies inside the third sequence: no entry over a
    # junction, and nothing matches x there
    x = mer(rng, k)
    out["four_sequences"] = [S.dna(rng, X.ref_len_for_windows(X.SPAN, k, w) - k // 2) + x[:k // 2], x[k // 2:] + S.dna(rng, 200), b"",
                             S.dna(rng, 150) + revcomp(x) + S.dna(rng, 150) + b"A" * 40, b"A" * 40 + S.dna(rng, 90)]
    return out


# ------------------------------------------------------------------ the read sketch
READ_WINDOWS = (63, 64, 65, 129)   # the chunk edges


def read_cases(k: int, w: int, seed: int = 89):
    """-> (sequences, Reads): reads of 0, k - 1 and k bytes, reads with READ_WINDOWS windows drawn from either strand of the reference,
    one with lower case and other bytes, one of inverted repeats and one rich in palindromes."""
    rng = np.random.default_rng(seed + 100 * k + w)
    ref = S.dna(rng, 900)
    reads = [b"", ref[:k - 1], ref[5:5 + k]]
    for n, nw in enumerate(READ_WINDOWS):
        L = X.ref_len_for_windows(nw, k, w)
        q = S.mutate(rng, ref[40 * n:40 * n + L + 8], 0.03)[:L]
        q += S.dna(rng, L - len(q))
        reads.append(revcomp(q) if n % 2 else q)
    low = bytearray(ref[300:520].lower())
    low[50], low[51], low[130] = ord("N"), ord("n"), ord("-")
    rep = inverted_repeats(rng, k, w, 12)
    reads += [bytes(low), rep, b"ACGT" * 30 + ref[600:640]]
    return [ref[:450], ref[450:] + rep[:len(rep) // 2] + b"ACGT" * 10], Reads(reads)


# ------------------------------------------------------------------ the lookup
def strands_case(seed: int = 97):
    """k 11, w 3 -> (sequences, Reads): a read of more than 64 entries whose first half comes from the plus strand of the reference and
    whose second half from the minus strand -- the sorted entries mix them, so every step of 64 has hits of both problems --, a read with
    minus hits only and a read with no hits."""
    rng = np.random.default_rng(seed)
    ref = S.dna(rng, 1500)
    both = S.mutate(rng, ref[100:400], 0.03) + revcomp(S.mutate(rng, ref[800:1100], 0.03))
    return [ref[:700], ref[700:]], Reads([both, revcomp(ref[1200:1450]), S.dna(rng, 200)])


def occ_case(k: int, max_occ: int, max_ref_occ: int, seed: int = 101):
    """With w = 1, in the manner of index_ref.occ_case: four k-mers that the reference holds max_ref_occ or max_ref_occ + 1 times and the
    read max_occ or max_occ + 1 times, every group split across the strands -- n times means n - 1 copies and one reverse complement
    (for n = 1 the one copy) -- so that a cap counted per strand lets the groups just over a cap through."""
    rng = np.random.default_rng(seed)
    gap = lambda: S.dna(rng, 31)   # noqa: E731
    put = lambda x, n: b"".join(b"N" + y + b"N" + gap() for y in [x] * (n - 1 if n > 1 else 1) + [revcomp(x)] * (1 if n > 1 else 0))   # noqa: E731
    ref, read = gap(), gap()
    for in_ref, in_read in ((max_ref_occ, max_occ), (max_ref_occ + 1, max_occ), (max_ref_occ, max_occ + 1), (max_ref_occ + 1, max_occ + 1)):
        x = mer(rng, k)
        ref += put(x, in_ref)
        read += put(x, in_read)
    return [ref], Reads([read, revcomp(read), read[:len(read) // 2]])


OCC_CAPS = ((1, 1), (2, 3), (64, 2))


def hit_sort_case(extra: int, k: int = 12):
    """index_ref.hit_sort_case with its big read reverse-complemented: a minus problem with SORT_LDS + extra hits, w = 1."""
    ref, rs = X.hit_sort_case(extra, k)
    small = [q for q, s in rs.reads if s == 0]
    return [ref], Reads([small[0], small[1], revcomp(small[2]), small[3]])


# ------------------------------------------------------------------ the tie to the listed-twice path
def tie_case(k: int, seed: int = 103, n: int = 6):
    """With w = 1 and no caps -> (sequences, Reads): reads drawn from the reference with edits, half from the minus strand, one with an N."""
    rng = np.random.default_rng(seed + k)
    ref = S.dna(rng, 1200)
    reads = []
    for i in range(n):
        a = int(rng.integers(0, 900))
        q = S.mutate(rng, ref[a:a + int(rng.integers(60, 300))], 0.04)
        if i == 1:
            q = q[:30] + b"N" + q[31:]
        reads.append(revcomp(q) if i % 2 else q)
    return [ref[:500], ref[500:]], Reads(reads)


# ------------------------------------------------------------------ the whole path
MAP_PARAMS = Params(13, 8, 16, 32)
MAP_LENGTHS = (8000, 2500, 0, 9500)
MAP_NAMES = ("chr_a", "contig_b", "nothing", "chr_d")
MAP_READS = 24


class BothMappingSet:
    """Four sequences of 20 kbp in all and 24 reads of 1 .. 2 kbp with 5 % edits, every other one from the minus strand, each listed once.
    The last read is chimeric: its first half is the end of the 2500-base sequence, its second half the start of the 9500-base one, which are
    adjacent in the index's frame. origin[i] = (seq, start, end, strand) in the sequence's own coordinates; the chimeric read has none.
    reads: the reads once (what the seeder takes); twice: the 2 n problems, for the models that take one problem per strand."""

    def __init__(self, seed: int = 107):
        rng = np.random.default_rng(seed)
        self.seqs = [S.dna(rng, n) for n in MAP_LENGTHS]
        self.start = M.seq_start(self.seqs)
        reads, self.origin = [], []
        for i in range(MAP_READS - 1):
            s = (0, 3, 1)[i % 3] if i % 6 != 5 else 3
            L = int(rng.integers(1000, 2001))
            a = int(rng.integers(0, MAP_LENGTHS[s] - L))
            reads.append(S.oriented(S.mutate(rng, self.seqs[s][a:a + L], 0.05), i % 2))
            self.origin.append((s, a, a + L, i % 2))
        reads.append(S.mutate(rng, self.seqs[1][-700:] + self.seqs[3][:800], 0.05))
        self.chimeric = MAP_READS - 1
        self.once = Reads(reads)
        order = (3, 0, 2, 1)   # the caller's pool: the reads, then the sequences in another order and apart from one another
        off, pool = {}, self.once.pool.tobytes()
        for s in order:
            pool += b"#" * 5
            off[s] = len(pool)
            pool += self.seqs[s]
        self.pool = np.frombuffer(pool + b"#" * 8, np.uint8).copy()
        self.seq_off = np.array([off[s] for s in range(len(self.seqs))], np.uint64)
        self.seq_len = np.array(MAP_LENGTHS, np.uint32)
        self.reads = self.once.listed_twice()   # (index_multi_ref.windowed_chain_set reads the problems from here)

    def true_problem(self, i: int) -> int:
        return 2 * i + self.origin[i][3]

    def expected_hits(self):
        return per_problem(expected(self.once.reads, self.seqs, MAP_PARAMS))
