"""The rule of INTEGRATION.md, "Selecting a read's alignments", as a Python model: position by position, plain integers, no NumPy tricks.
The selector's kernels (ba_select.hip) equal it bit for bit. Also the known answer of that chapter and the sets of the GPU tests."""
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "mask_permille sec_permille max_secondary mapq_max full_support min_score")
PRIMARY, SUPPLEMENTARY, SECONDARY, DROPPED, EXCLUDED = 0, 1, 2, 3, 4
NONE = 0xffffffff
MAX_PER_READ = 1024

KNOWN_PARAMS = Params(500, 800, 2, 60, 10, 20)
KNOWN = dict(read=[0, 0, 0, 0, 0, 0, 0, 1, 0, 1],
             q_len=[1000, 1000, 1000, 1000, 1000, 1000, 1000, 400, 1000, 400],
             score=[300, 500, 480, 90, 410, 405, 15, 200, 120, 200],
             q_start=[600, 0, 20, 650, 100, 580, 0, 0, 520, 10],
             q_end=[1000, 500, 520, 900, 450, 980, 50, 400, 1000, 390],
             strand=[0, 0, 1, 0, 0, 1, 0, 1, 0, 0],
             support=[12, 30, 9, 3, 8, 8, 1, 4, 5, 20])
KNOWN_OUT = dict(cls=[3, 0, 1, 3, 2, 2, 4, 0, 3, 2],
                 mapq=[0, 10, 20, 0, 0, 0, 0, 0, 0, 0],
                 parent=[2, 1, 2, 2, 1, 1, NONE, 7, 2, 7],
                 rank=[4, 0, 1, 6, 2, 3, NONE, 0, 5, 1],
                 sub_score=[0, 410, 300, 0, 0, 0, 0, 200, 0, 0],
                 kept=[1, 2, 4, 5, 7, 9],
                 kept_first=[0, 4, 6],
                 kept_per_read=[4, 2])


def select(P: Params, read, score, q_start, q_end, q_len, strand=None, support=None, exclude=None, n_reads=None):
    """-> dict of lists: cls, mapq, parent, rank, sub_score per candidate in the caller's order; kept_first, kept, kept_per_read."""
    n = len(read)
    read = [int(x) for x in read]
    if n_reads is None:
        n_reads = max(read) + 1 if n else 0
    cls, mapq, parent, rank, sub_score = [EXCLUDED] * n, [0] * n, [NONE] * n, [NONE] * n, [0] * n
    a, b = [0] * n, [0] * n
    members = [[] for _ in range(n_reads)]
    for c in range(n):
        minus = 0 if strand is None else int(strand[c])
        qs, qe, ql, s = int(q_start[c]), int(q_end[c]), int(q_len[c]), int(score[c])
        assert qs <= qe <= ql and minus in (0, 1) and read[c] < n_reads
        a[c] = ql - qe if minus else qs
        b[c] = ql - qs if minus else qe
        if (exclude is None or not int(exclude[c])) and s >= P.min_score and b[c] - a[c] > 0:
            members[read[c]].append(c)
    kept_first, kept, kept_per_read = [0], [], []
    for r in range(n_reads):
        order = sorted(members[r], key=lambda c: (-int(score[c]), c))
        heads, sub, secondaries = [], {}, 0
        for i, c in enumerate(order):
            rank[c] = i
            s = int(score[c])
            found = None
            for h in heads:
                ov = min(b[c], b[h]) - max(a[c], a[h])
                if ov > 0 and 1000 * ov >= P.mask_permille * min(b[c] - a[c], b[h] - a[h]):
                    found = h
                    break
            if found is None:
                heads.append(c)
                sub[c] = 0
                parent[c] = c
                cls[c] = PRIMARY if i == 0 else SUPPLEMENTARY
                continue
            parent[c] = found
            sub[found] = max(sub[found], s)
            if 1000 * s >= P.sec_permille * int(score[found]) and secondaries < P.max_secondary:
                cls[c] = SECONDARY
                secondaries += 1
            else:
                cls[c] = DROPPED
        for h in heads:
            s1, s2 = int(score[h]), sub[h]
            u = P.full_support if support is None else min(int(support[h]), P.full_support)
            mapq[h] = (P.mapq_max * (s1 - s2) * u) // (s1 * P.full_support)
            sub_score[h] = s2
        mine = [c for c in order if cls[c] <= SECONDARY]
        kept += mine
        kept_per_read.append(len(mine))
        kept_first.append(len(kept))
    return dict(cls=cls, mapq=mapq, parent=parent, rank=rank, sub_score=sub_score, kept_first=kept_first, kept=kept, kept_per_read=kept_per_read)


# ------------------------------------------------------------------ candidate sets
class CandidateSet:
    """Candidates in the layout ba_select_create takes (strand, support and exclude may be None)."""

    def __init__(self, read, score, q_start, q_end, q_len, strand=None, support=None, exclude=None, n_reads=None):
        u32 = lambda x: np.asarray(x, np.uint32)
        self.read, self.score = u32(read), np.asarray(score, np.int32)
        self.q_start, self.q_end, self.q_len = u32(q_start), u32(q_end), u32(q_len)
        self.strand = None if strand is None else np.asarray(strand, np.uint8)
        self.support = None if support is None else u32(support)
        self.exclude = None if exclude is None else np.asarray(exclude, np.uint8)
        self.n_reads = int(self.read.max()) + 1 if n_reads is None else n_reads

    def __len__(self):
        return len(self.read)

    def args(self):
        return (self.read, self.score, self.q_start, self.q_end, self.q_len, self.strand, self.support, self.exclude, self.n_reads)

    def expected(self, P: Params):
        return select(P, *self.args())

    def replace(self, **kw):
        d = dict(read=self.read, score=self.score, q_start=self.q_start, q_end=self.q_end, q_len=self.q_len, strand=self.strand,
                 support=self.support, exclude=self.exclude, n_reads=self.n_reads)
        d.update(kw)
        return CandidateSet(**d)

    def permuted(self, perm):
        pick = lambda x: None if x is None else x[perm]
        return CandidateSet(self.read[perm], self.score[perm], self.q_start[perm], self.q_end[perm], self.q_len[perm], pick(self.strand),
                            pick(self.support), pick(self.exclude), self.n_reads)


def known_set() -> CandidateSet:
    return CandidateSet(**KNOWN)


def random_read(rng, r, n, q_len=None, distinct_scores=False, p_exclude=0.05, low=0.1):
    """n candidates of read r: spans drawn around a few loci of a read, so that many overlap and many do not; scores from 1 (some below any min_score);
    both strands; a few empty spans and a few excluded. -> list of rows (read, score, q_start, q_end, q_len, strand, support, exclude)."""
    ql = int(rng.integers(50, 20000)) if q_len is None else q_len
    loci = [int(rng.integers(0, ql)) for _ in range(1 + n // 2)]
    scores = rng.permutation(np.arange(30, 30 + 3 * n))[:n].tolist() if distinct_scores else rng.integers(30, 30 + max(4, n // 2), n).tolist()
    rows = []
    for k in range(n):
        mid, half = loci[int(rng.integers(0, len(loci)))], int(rng.integers(0, max(2, ql // (2 * len(loci)))))
        qs, qe = max(0, mid - half), min(ql, mid + int(rng.integers(0, half + 1)))
        if qe < qs:
            qe = qs
        s = int(rng.integers(1, 20)) if rng.random() < low else int(scores[k])
        rows.append((r, s, qs, qe, ql, int(rng.integers(0, 2)), int(rng.integers(1, 40)), int(rng.random() < p_exclude)))
    return rows


def from_rows(rows, n_reads=None, shuffle=None) -> CandidateSet:
    if shuffle is not None:
        rows = [rows[i] for i in shuffle.permutation(len(rows))]
    cols = list(zip(*rows)) if rows else [[]] * 8
    return CandidateSet(*cols, n_reads=n_reads)


def disjoint_read(r, n=130, width=10):
    """n pairwise disjoint spans of one read: every candidate becomes a head."""
    return [(r, 1000 - k, k * width, k * width + width - 1, n * width, 0, 5 + k % 9, 0) for k in range(n)]


def tie_read(rng, r, n=100, score=77):
    """Every candidate has the same score: the index decides the order."""
    return [(row[0], score) + row[2:7] + (0,) for row in random_read(rng, r, n, low=0.0)]


SIZES = (0, 1, 2, 63, 64, 65, 200, 1024)
GPU_PARAMS = Params(500, 800, 5, 60, 10, 20)
MAX_SECONDARY = (0, 1, 64)
MASK_PERMILLE = (1, 1000)
SEC_PERMILLE = (0, 1000)


def gpu_sets():
    """The candidate sets of tests/test_gpu_select.py, by name (tests/test_select_ref.py asserts on the CPU what they are meant to hold)."""
    rng = np.random.default_rng(4711)
    sizes = [row for r, n in enumerate(SIZES) for row in random_read(rng, r, n)]
    special = disjoint_read(0) + tie_read(rng, 1) + [row[:7] + (1,) for row in random_read(rng, 2, 40)] + random_read(rng, 3, 90, distinct_scores=True)
    many = [row for r in range(3000) for row in random_read(rng, r, int(rng.integers(1, 5)), q_len=int(rng.integers(40, 3000)))]
    smaller = [row for r, n in enumerate((30, 0, 64, 7)) for row in random_read(rng, r, n)]
    return dict(known=known_set(), sizes=from_rows(sizes, len(SIZES), rng), special=from_rows(special, 4, rng), many=from_rows(many, 3000, rng),
                smaller=from_rows(smaller, 4, rng))
