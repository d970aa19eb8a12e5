"""A model of minimizer seeding ("Seeding"): the (w, k)-minimizer sketch of a sequence, the hits of a problem and the strand
frame, all in integers, and the problem sets the GPU tests compare Seeder with. The rule is written twice: sketch_plain() / hits_plain() spell
it out position by position in plain Python, sketch() / hits() are the same in NumPy for the long sequences; tests/test_seeding_ref.py holds
one against the other. hits() is what ba_seeding_* must report for one problem, bit for bit."""
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "k w max_occ")
NO_CAP = 0xffffffff
MASK = 0xffffffff

HASH_CHECKS = {0: 0x92ca2f0e, 1: 0x36deb503, 0x1b: 0xd550a319, 0xffffffff: 0x3b66b2aa}

KNOWN_R = b"TTACGTTGCATGGACGTAGGATCCAGTCACGTTGCA"
KNOWN_Q = b"ACGTTGCATGGACCTAGGATCCAGTnACGTTGCATGGA"          # strand 0, k 5, w 4
KNOWN_Q_SKETCH = [3, 5, 8, 11, 12, 16, 19, 20, 26, 27, 29, 31]
KNOWN_R_SKETCH = [0, 3, 5, 7, 10, 12, 16, 18, 21, 24, 27, 31]
KNOWN_HITS_OCC2 = [(27, 3), (3, 5), (29, 5), (5, 7), (31, 7), (8, 10), (16, 18), (19, 21), (3, 31), (29, 31)]
KNOWN_HITS_OCC1 = [(27, 3), (8, 10), (16, 18), (19, 21)]
KNOWN_Q_MINUS = b"TCCATGCAACGTNACTGGATCC"                       # strand 1, k 5, w 3, max_occ 4, against KNOWN_R
KNOWN_Q_MINUS_SKETCH = [0, 3, 4, 10, 11, 13, 15]
KNOWN_HITS_MINUS = [(11, 3), (13, 5), (15, 7), (0, 18), (3, 21), (11, 29), (13, 31)]

_CODE = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3, ord("a"): 0, ord("c"): 1, ord("g"): 2, ord("t"): 3}
_COMP = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C")}


def h32(x: int) -> int:
    x = (x ^ 0x9e3779b9) & MASK
    x ^= x >> 16
    x = (x * 0x85ebca6b) & MASK
    x ^= x >> 13
    x = (x * 0xc2b2ae35) & MASK
    x ^= x >> 16
    return x


def upper(c: int) -> int:
    return c - 32 if ord("a") <= c <= ord("z") else c


def oriented(q: bytes, strand: int) -> bytes:
    """The query in the chain batch's frame: with strand 1 its reverse complement (uppercased, A<->T, C<->G, every other byte as it is)."""
    if not strand:
        return bytes(q)
    return bytes(_COMP.get(upper(c), upper(c)) for c in reversed(bytes(q)))


# ------------------------------------------------------------------ the rule, position by position
def codes_plain(seq: bytes, k: int):
    """-> the code of every k-mer, None for an invalid one."""
    out = []
    for i in range(len(seq) - k + 1):
        c = 0
        for t in range(k):
            b = _CODE.get(seq[i + t])
            if b is None:
                c = None
                break
            c = c << 2 | b
        out.append(c)
    return out


def sketch_plain(seq: bytes, k: int, w: int):
    """-> (positions, codes) of the selected k-mers, ascending by position."""
    cs = codes_plain(seq, k)
    nk = len(cs)
    if nk == 0:
        return [], []
    windows = [(0, nk)] if nk <= w else [(s, s + w) for s in range(nk - w + 1)]
    sel = set()
    for a, b in windows:
        best = None
        for i in range(a, b):
            if cs[i] is not None and (best is None or h32(cs[i]) < h32(cs[best])):   # (strictly smaller: the leftmost of equals stays)
                best = i
        if best is not None:
            sel.add(best)
    pos = sorted(sel)
    return pos, [cs[i] for i in pos]


def hits_plain(q: bytes, r: bytes, P: Params, strand: int = 0):
    """-> [(q_hit, r_hit)] of one problem, in the order of the rule."""
    qp, qc = sketch_plain(oriented(q, strand), P.k, P.w)
    rp, rc = sketch_plain(bytes(r), P.k, P.w)
    index = {}
    for i, c in zip(qp, qc):
        index.setdefault(c, []).append(i)
    out = []
    for j, c in zip(rp, rc):
        m = index.get(c, [])
        if 1 <= len(m) <= P.max_occ:
            out += [(i, j) for i in m]
    return out


def brute_force_hits(q: bytes, r: bytes, k: int, strand: int = 0):
    """Every shared valid k-mer of the oriented query and the reference, sorted by (r, q): what w = 1 without a cap must give."""
    qo = oriented(q, strand).upper()
    ro = bytes(r).upper()
    ok = set(b"ACGT")
    out = []
    for j in range(len(ro) - k + 1):
        if not set(ro[j:j + k]) <= ok:
            continue
        for i in range(len(qo) - k + 1):
            if qo[i:i + k] == ro[j:j + k]:
                out.append((i, j))
    return out


# ------------------------------------------------------------------ the same in NumPy
_LUT = np.full(256, 4, np.uint8)
for _b, _v in _CODE.items():
    _LUT[_b] = _v


def h32_np(x):
    x = x.astype(np.uint64)
    x = (x ^ np.uint64(0x9e3779b9)) & np.uint64(MASK)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85ebca6b)) & np.uint64(MASK)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xc2b2ae35)) & np.uint64(MASK)
    x ^= x >> np.uint64(16)
    return x


def sketch(seq: bytes, k: int, w: int):
    """-> (positions, codes) as uint32 arrays, ascending by position."""
    two = _LUT[np.frombuffer(bytes(seq), np.uint8)]
    nk = len(two) - k + 1
    if nk <= 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    code = np.zeros(nk, np.uint64)
    bad = np.zeros(nk, bool)
    for t in range(k):
        x = two[t:t + nk]
        bad |= x > 3
        code = code << np.uint64(2) | (x & 3).astype(np.uint64)
    key = h32_np(code) << np.uint64(32) | np.arange(nk, dtype=np.uint64)
    key[bad] = np.uint64(0xffffffffffffffff)
    if nk <= w:
        mins = key.min(keepdims=True)
    else:
        mins = np.lib.stride_tricks.sliding_window_view(key, w).min(axis=1)
    mins = np.unique(mins[mins != np.uint64(0xffffffffffffffff)])
    pos = np.sort((mins & np.uint64(MASK)).astype(np.int64))
    return pos.astype(np.uint32), code[pos].astype(np.uint32)


def hits(q: bytes, r: bytes, P: Params, strand: int = 0):
    """-> dict(q_pos, q_code, r_pos, r_code: the sketches; q_hit, r_hit: the hits) of one problem, uint32 arrays."""
    qp, qc = sketch(oriented(q, strand), P.k, P.w)
    rp, rc = sketch(bytes(r), P.k, P.w)
    qkey = np.sort(qc.astype(np.uint64) << np.uint64(32) | qp.astype(np.uint64))
    lo = np.searchsorted(qkey, rc.astype(np.uint64) << np.uint64(32), "left")
    hi = np.searchsorted(qkey, rc.astype(np.uint64) << np.uint64(32) | np.uint64(MASK), "left")   # (no position is 0xffffffff; code + 1 can leave 64 bits)
    m = hi - lo
    m[m > P.max_occ] = 0
    at = np.repeat(lo, m) + (np.arange(int(m.sum())) - np.repeat(np.cumsum(m) - m, m))
    return dict(q_pos=qp, q_code=qc, r_pos=rp, r_code=rc,
                q_hit=(qkey[at] & np.uint64(MASK)).astype(np.uint32), r_hit=np.repeat(rp, m).astype(np.uint32))


# ------------------------------------------------------------------ problem sets
class ProblemSet:
    """Problems in the layout ba_seeding_create takes: pairs [(q, r)] or [(q, r, strand)] of byte strings, packed into one pool."""

    def __init__(self, pairs):
        self.pairs = [(bytes(p[0]), bytes(p[1]), int(p[2]) if len(p) > 2 else 0) for p in pairs]
        seqs = [s for p in self.pairs for s in p[:2]]
        lens = np.array([len(s) for s in seqs], np.int64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(seqs) else np.zeros(0, np.int64)
        self.pool = np.frombuffer(b"".join(seqs) + b"#", np.uint8).copy()   # (one byte more: an empty pool has no address)
        self.q_off, self.r_off = offs[0::2].astype(np.uint64), offs[1::2].astype(np.uint64)
        self.q_len, self.r_len = lens[0::2].astype(np.uint32), lens[1::2].astype(np.uint32)
        self.strand = np.array([p[2] for p in self.pairs], np.uint8)

    def __len__(self):
        return len(self.pairs)

    def args(self):
        return (self.pool, self.q_off, self.q_len, self.r_off, self.r_len, self.strand)

    def expected(self, P: Params):
        return [hits(q, r, P, s) for q, r, s in self.pairs]


def dna(rng, n: int) -> bytes:
    return bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))


def mutate(rng, s: bytes, rate: float) -> bytes:
    """Substitutions, insertions and deletions at `rate` per base."""
    out = bytearray()
    for c in s:
        x = rng.random()
        if x < rate / 3:
            continue
        if x < 2 * rate / 3:
            out += dna(rng, 1)
        if x < rate:
            out += dna(rng, 1)
        else:
            out.append(c)
    return bytes(out)


def edge_lengths(k: int, w: int):
    """The lengths at which the sketch takes another path: no k-mer, one, one window, two, and the chunk (64 windows) and halo boundaries."""
    return sorted({0, k - 1, k, k + 1, k + w - 2, k + w - 1, k + w} | {x + k for x in (62, 63, 64, 65, 66, 126, 127, 128, 129, 130)})


EDGE_K = (4, 15, 16)
EDGE_W = (1, 2, 16, 63, 64)
SORT_ENTRIES = (1, 2, 63, 64, 65, 8191, 8192, 8193, 20000)


def lengths_set(k: int, w: int, seed: int = 7):
    """The edge lengths on either side against a mutated copy of another edge length, and an empty query and an empty reference."""
    rng = np.random.default_rng(seed + 100 * k + w)
    Ls = edge_lengths(k, w)
    pairs = []
    for n, L in enumerate(Ls):
        base = dna(rng, max(L, Ls[-1 - n]) + 8)
        pairs.append((base[:L], mutate(rng, base, 0.03)[:Ls[-1 - n]], n % 2))
    pairs += [(b"", dna(rng, 90)), (dna(rng, 90), b"")]
    return ProblemSet(pairs)


def other_bytes_set(k: int, w: int, seed: int = 11):
    """Bytes outside ACGT: an N first, last, at every k-th position (no valid k-mer), a run longer than k + w (whole windows select
    nothing), and lower case."""
    rng = np.random.default_rng(seed)
    base = dna(rng, 400)
    first, last = b"N" + base[1:], base[:-1] + b"N"
    every = bytearray(base)
    every[k - 1::k] = b"N" * len(every[k - 1::k])
    run = base[:150] + b"N" * (k + w + 3) + base[150:]
    two_runs = base[:70] + b"-" * (2 * (k + w)) + base[70:200] + b"n" * (k + w + 1) + base[200:]
    lower = base.lower()
    mixed = bytes(c + 32 if rng.random() < 0.5 else c for c in base)
    return ProblemSet([(first, base), (base, last), (bytes(every), base), (base, bytes(every)), (run, base), (base, run, 1), (two_runs, run),
                       (lower, base), (base, mixed), (mixed, lower, 1), (b"N" * 200, base), (base, b"N" * 200)])


def tie_set():
    """Equal hashes in every window: a homopolymer and an AC tandem repeat of 300 bases, against themselves and one another."""
    a, ac = b"A" * 300, b"AC" * 150
    return ProblemSet([(a, a), (ac, ac), (a, ac), (ac, a, 1), (a, b"T" * 300, 1), (ac, b"GT" * 150, 1)])


def occ_set(k: int, max_occ: int, seed: int = 13):
    """With w = 1: a k-mer that the query holds exactly max_occ and max_occ + 1 times, between unrelated stretches (every k-mer is selected,
    so the occurrences among the selected entries are the occurrences in the sequence)."""
    rng = np.random.default_rng(seed)
    mer, other = dna(rng, k), dna(rng, k)
    gap = lambda: dna(rng, 37)   # noqa: E731
    q_at = b"".join(gap() + mer for _ in range(max_occ)) + gap()
    q_over = b"".join(gap() + other for _ in range(max_occ + 1)) + gap()
    r = gap() + mer + gap() + other + gap() + mer + gap()
    return ProblemSet([(q_at, r), (q_over, r), (q_at + q_over, r), (oriented(q_at + q_over, 1), r, 1)])


def sort_set(k: int = 15, seed: int = 17):
    """With w = 1: queries of SORT_ENTRIES entries (length entries + k - 1) against short copies of stretches of them, so that the searches
    meet duplicated codes."""
    rng = np.random.default_rng(seed)
    pairs = []
    for n in SORT_ENTRIES:
        q = dna(rng, n + k - 1)
        if n >= 200:   # a stretch twice in the query: codes that occur twice
            q = q[:100] + q[:60] + q[160:]
        r = q[:min(len(q), 120)] + q[-min(len(q), 80):] + q[len(q) // 2:len(q) // 2 + 50]
        pairs.append((q, r))
    return ProblemSet(pairs)


def long_reference_set(seed: int = 19):
    """A 70 kbp reference against a 500-base read cut out of it, and the same on the minus strand."""
    rng = np.random.default_rng(seed)
    ref = dna(rng, 70000)
    read = mutate(rng, ref[41000:41500], 0.05)
    return ProblemSet([(read, ref), (oriented(read, 1), ref, 1)])


def tiny_set(n: int = 2000, seed: int = 23):
    """n problems of 0 .. 60 bases a side, every fifth with an empty side."""
    rng = np.random.default_rng(seed)
    pairs = []
    for p in range(n):
        base = dna(rng, int(rng.integers(10, 61)))
        q, r = mutate(rng, base, 0.05), base
        if p % 5 == 0:
            q, r = (b"", r) if p % 10 == 0 else (q, b"")
        pairs.append((q, r, int(rng.integers(0, 2))))
    return ProblemSet(pairs)


def strand_set(seed: int = 29):
    """Mixed strands, and the same read listed on both strands against the same reference (the pool is shared: the offsets repeat)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for p in range(12):
        ref = dna(rng, int(rng.integers(150, 400)))
        read = mutate(rng, ref[20:-20], 0.06)
        pairs.append((oriented(read, p % 2), ref, p % 2))
    ps = ProblemSet(pairs)
    # problem 0's read on both strands, and problem 1's: appended as rows that point at the same bytes
    for p in (0, 1):
        for s in (0, 1):
            ps.pairs.append((ps.pairs[p][0], ps.pairs[p][1], s))
            ps.q_off, ps.q_len = np.append(ps.q_off, ps.q_off[p]), np.append(ps.q_len, ps.q_len[p])
            ps.r_off, ps.r_len = np.append(ps.r_off, ps.r_off[p]), np.append(ps.r_len, ps.r_len[p])
            ps.strand = np.append(ps.strand, np.uint8(s))
    return ps


def smaller_set(seed: int = 31):
    rng = np.random.default_rng(seed)
    pairs = []
    for n in (80, 0, 33):
        base = dna(rng, n)
        pairs.append((mutate(rng, base, 0.04), base))
    return ProblemSet(pairs)


def over_limit_set():
    """A 17 000-base poly-A against itself: with w 1 and no cap 16 986 x 16 986 hits, more than 2^28."""
    a = b"A" * 17000
    return ProblemSet([(b"ACGTACGTACGTACGTACGT", b"ACGTACGTACGTACGTACGT"), (a, a), (b"ACGTTGCATGGACCTAGGATCCAGT", b"GGACCTAGGATCCAGTACGTTGCAT")])


PIPELINE_PARAMS = Params(10, 5, 8)


def chain_set_problems(cs):
    """A tests/chain_ref.py chain set's reads as seeding problems (the set's own pool and per-chain arrays) -> (args, [(q, r, strand)])."""
    strand = np.array([c[3] for c in cs.chains], np.uint8)
    cut = lambda off, ln: cs.pool[int(off):int(off) + int(ln)].tobytes()   # noqa: E731
    pairs = [(cut(cs.q_off[c], cs.q_len[c]), cut(cs.r_off[c], cs.r_len[c]), int(strand[c])) for c in range(len(cs))]
    return (cs.pool, cs.q_off, cs.q_len, cs.r_off, cs.r_len, strand), pairs
