"""Models of the reference index ("Reference index"), in integers: the index's entries, the hits of a read against the whole
indexed reference -- the rule of tests/seeding_ref.py plus the cap on a code's occurrences in the reference's sketch --, and the candidate
windows of chains. hits() is what an indexed Seeder must report for one problem, bit for bit; chain_windows() what ba_chain_windows writes.
Also the read set that the CPU and the GPU test of the whole path share."""
from collections import namedtuple

import numpy as np

from tests import chain_ref, chaining_ref, seeding_ref as S

Params = namedtuple("Params", "k w max_occ max_ref_occ")
NO_CAP = S.NO_CAP
SPAN = 1024             # ba::INDEX_SPAN (ba_index.h): windows per work item of k_index_sketch
SORT_LDS = 8192         # ba::SEEDING_SORT_LDS


def entries(ref: bytes, k: int, w: int):
    """-> (code, pos) of the index, ascending by (code, pos), and longest_run."""
    pos, code = S.sketch(bytes(ref), k, w)
    key = np.sort(code.astype(np.uint64) << np.uint64(32) | pos.astype(np.uint64))
    code = (key >> np.uint64(32)).astype(np.uint32)
    longest = int(np.unique(code, return_counts=True)[1].max()) if len(code) else 0
    return code, (key & np.uint64(S.MASK)).astype(np.uint32), longest


def hits(q: bytes, ref: bytes, P: Params, strand: int = 0):
    """The plain rule with r the whole reference, then the reference cap: a hit stays if the code of its reference entry occurs at most
    max_ref_occ times in the reference's sketch -> dict(q_pos, q_code, q_hit, r_hit)."""
    e = S.hits(q, ref, S.Params(P.k, P.w, P.max_occ), strand)
    codes, counts = np.unique(e["r_code"], return_counts=True)
    occ = dict(zip(codes.tolist(), counts.tolist()))
    code_at = dict(zip(e["r_pos"].tolist(), e["r_code"].tolist()))
    keep = np.array([occ[code_at[j]] <= P.max_ref_occ for j in e["r_hit"].tolist()], bool)
    return dict(q_pos=e["q_pos"], q_code=e["q_code"], q_hit=e["q_hit"][keep], r_hit=e["r_hit"][keep])


def hits_plain(q: bytes, ref: bytes, P: Params, strand: int = 0):
    """The same position by position -> [(q_hit, r_hit)]."""
    rp, rc = S.sketch_plain(bytes(ref), P.k, P.w)
    code_at = dict(zip(rp, rc))
    return [(i, j) for i, j in S.hits_plain(q, ref, S.Params(P.k, P.w, P.max_occ), strand) if rc.count(code_at[j]) <= P.max_ref_occ]


def chain_windows(q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, margin: int):
    """-> (r_off, r_len, r_anchor, shift) as ba_chain_windows writes them, in Python's integers."""
    r_off_w, r_len_w, r_anchor_w, shift = [], [], [int(x) for x in r_anchor], []
    for c in range(len(q_len)):
        a0, a1 = int(anchor_first[c]), int(anchor_first[c + 1])
        if a1 <= a0:
            raise ValueError(f"chain {c} has no anchors")
        for a in range(a0, a1):
            if int(q_anchor[a]) + int(anchor_len[a]) > int(q_len[c]) or int(r_anchor[a]) + int(anchor_len[a]) > int(r_len[c]):
                raise ValueError(f"chain {c}: anchor {a - a0} ends outside its sequences")
        qa0, ra0 = int(q_anchor[a0]), int(r_anchor[a0])
        qe, re = int(q_anchor[a1 - 1]) + int(anchor_len[a1 - 1]), int(r_anchor[a1 - 1]) + int(anchor_len[a1 - 1])
        lo = ra0 - min(ra0, qa0 + margin)
        hi = re + min(int(r_len[c]) - re, (int(q_len[c]) - qe) + margin)
        r_off_w.append(int(r_off[c]) + lo)
        r_len_w.append(hi - lo)
        shift.append(lo)
        for a in range(a0, a1):
            r_anchor_w[a] -= lo
    return np.array(r_off_w, np.uint64), np.array(r_len_w, np.uint32), np.array(r_anchor_w, np.uint32), np.array(shift, np.uint64)


# ------------------------------------------------------------------ references around the seams of the sketch
def ref_len_for_windows(nw: int, k: int, w: int) -> int:
    """The length of a sequence with nw > 1 windows: nk = nw + w - 1 k-mers."""
    return nw + w - 1 + k - 1


SEAM_WINDOWS = (SPAN - 1, SPAN, SPAN + 1, 2 * SPAN + 1)
SEAM_KW = ((4, 1), (15, 10), (16, 64))


def seam_references(k: int, w: int, seed: int = 41):
    """-> {name: bytes}: random DNA with every window count of SEAM_WINDOWS; a poly-A run and a run of N longer than k + w across the first
    seam (window SPAN starts at byte SPAN); the all-T 16-mer; and the short ones: no k-mer, one k-mer, one window."""
    rng = np.random.default_rng(seed + 100 * k + w)
    out = {f"random_{nw}": S.dna(rng, ref_len_for_windows(nw, k, w)) for nw in SEAM_WINDOWS}
    base = S.dna(rng, ref_len_for_windows(2 * SPAN + 1, k, w))
    run = k + w + 40
    at = SPAN - run // 2
    out["poly_a"] = base[:at] + b"A" * run + base[at + run:]
    out["n_run"] = base[:at] + b"N" * run + base[at + run:]
    out["n_run_ends_at_the_seam"] = base[:SPAN - run] + b"N" * run + base[SPAN:]
    out["all_t"] = base[:SPAN - 8] + b"T" * (run - 32) + base[SPAN - 8 + run - 32:]   # (a whole window of it: it is selected)
    out["shorter_than_k"] = base[:k - 1]
    out["exactly_k"] = base[:k]
    out["one_window"] = base[:k + w - 1]        # nk = w
    out["fewer_k_mers_than_w"] = base[:k + max(w - 2, 0)]
    out["empty"] = b""
    return out


# ------------------------------------------------------------------ reads against one reference
class ReadSet:
    """Reads in the layout ba_seeding_create_indexed takes: [(read, strand)] packed into one pool; the reference is not in it."""

    def __init__(self, reads):
        self.reads = [(bytes(q), int(s)) for q, s in reads]
        lens = np.array([len(q) for q, _ in self.reads], np.int64)
        self.pool = np.frombuffer(b"".join(q for q, _ in self.reads) + b"#", np.uint8).copy()
        self.q_off = (np.cumsum(lens) - lens).astype(np.uint64)
        self.q_len = lens.astype(np.uint32)
        self.strand = np.array([s for _, s in self.reads], np.uint8)

    def __len__(self):
        return len(self.reads)

    def args(self):
        return (self.pool, self.q_off, self.q_len, self.strand)

    def expected(self, ref: bytes, P: Params):
        return [hits(q, ref, P, s) for q, s in self.reads]

    def plain_args(self, ref: bytes):
        """The same problems for a plain Seeder: the reference appended to the pool, every problem's r all of it."""
        pool = np.concatenate([self.pool, np.frombuffer(bytes(ref) + b"#", np.uint8)])
        n = len(self)
        return (pool, self.q_off, self.q_len, np.full(n, len(self.pool), np.uint64), np.full(n, len(ref), np.uint32), self.strand)


def known_reads():
    """The known-answer strings of "Seeding" on both strands, a read without a valid k-mer and one without a hit."""
    return ReadSet([(S.KNOWN_Q, 0), (S.KNOWN_Q, 1), (S.KNOWN_Q_MINUS, 1), (S.KNOWN_Q_MINUS, 0), (b"ACGNACGNNACG", 0), (b"", 0), (b"CCCCCCCCCCCCC", 0)])


def occ_case(k: int, max_occ: int, max_ref_occ: int, seed: int = 43):
    """With w = 1 (every valid k-mer is selected): four k-mers that the reference holds max_ref_occ or max_ref_occ + 1 times and the read
    max_occ or max_occ + 1 times, between unrelated stretches -> (reference, ReadSet)."""
    rng = np.random.default_rng(seed)
    gap = lambda: S.dna(rng, 31)   # noqa: E731
    ref, read = gap(), gap()
    for in_ref, in_read in ((max_ref_occ, max_occ), (max_ref_occ + 1, max_occ), (max_ref_occ, max_occ + 1), (max_ref_occ + 1, max_occ + 1)):
        mer = S.dna(rng, k)
        ref += b"".join(b"N" + mer + b"N" + gap() for _ in range(in_ref))   # (the N: no k-mer over a border is shared by chance)
        read += b"".join(b"N" + mer + b"N" + gap() for _ in range(in_read))
    return ref, ReadSet([(read, 0), (S.oriented(read, 1), 1), (read[:len(read) // 2], 0)])


def hit_sort_case(extra: int, k: int = 12, seed: int = 47):
    """With w = 1: one k-mer 128 times in the reference and 64 times in the read, 128 * 64 = SORT_LDS hits, and `extra` more k-mers that
    both hold once; around them reads with 0, 1 and 2 hits -> (reference, ReadSet). The stretches between are unrelated and each k-mer is
    followed by its own separator, so that no other k-mer is shared."""
    rng = np.random.default_rng(seed)
    mer = S.dna(rng, k)
    uniq = [S.dna(rng, k) for _ in range(max(extra, 2))]
    ref = b"N".join([mer] * 128 + uniq) + b"N" + S.dna(rng, 200)
    big = b"N".join([mer] * 64 + uniq[:extra]) + b"N" + S.dna(rng, 150)
    return ref, ReadSet([(S.dna(rng, 90), 0), (uniq[0], 0), (big, 0), (uniq[0] + b"N" + uniq[1], 0), (S.oriented(big, 1), 1)])


# ------------------------------------------------------------------ the whole path: reads drawn from a reference
MAP_PARAMS = Params(11, 5, 16, 32)
MAP_CHAINING = chaining_ref.Params(4, 2, 0, 64, 400, 50, 2, 32, 1)
MAP_MARGIN = 64
MAP_SEED = 53


class MappingSet:
    """About 20 kbp of random DNA and 40 reads of 300 .. 1500 bases drawn from it with about 8 % edits, every other one from the minus
    strand; every read is listed on both strands: problem 2 i is read i on strand 0, problem 2 i + 1 on strand 1. origin[i] = (start, end,
    strand): where read i was drawn from."""

    def __init__(self, seed: int = MAP_SEED, ref_len: int = 20000, n: int = 40):
        rng = np.random.default_rng(seed)
        self.ref = S.dna(rng, ref_len)
        reads, self.origin = [], []
        for i in range(n):
            L = int(rng.integers(300, 1501))
            a = int(rng.integers(0, ref_len - L))
            read = S.mutate(rng, self.ref[a:a + L], 0.08)
            reads += [(S.oriented(read, i % 2), 0), (S.oriented(read, i % 2), 1)]
            self.origin.append((a, a + L, i % 2))
        self.reads = ReadSet(reads)

    def true_problem(self, i: int) -> int:
        return 2 * i + self.origin[i][2]


def model_chains(ms: MappingSet, exps):
    """The chaining model over the model's hits -> the chains as ba_chaining_results orders them: [(problem, rank, [(qa, ra, len)])]."""
    P = MAP_PARAMS
    cps = chaining_ref.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exps])
    out = []
    for p, res in enumerate(cps.expected(MAP_CHAINING)):
        for rank, (_, anchors) in enumerate(res["chains"]):
            out.append((p, rank, [(qa, ra, g) for qa, ra, g, _ in anchors]))
    return out


def windowed_chain_set(ms: MappingSet, chains, margin: int = MAP_MARGIN):
    """The chains cut to their candidate windows by the model, as a tests/chain_ref.py chain set whose references are the windows' bytes
    -> (ChainSet, shift)."""
    rs = ms.reads
    q_len = [int(rs.q_len[p]) for p, _, _ in chains]
    first = np.concatenate([[0], np.cumsum([len(a) for _, _, a in chains])])
    flat = [x for _, _, a in chains for x in a]
    r_off, r_len, r_anchor, shift = chain_windows(q_len, [0] * len(chains), [len(ms.ref)] * len(chains), first, [x[0] for x in flat],
                                                  [x[1] for x in flat], [x[2] for x in flat], margin)
    seqs = [q for q, _ in rs.reads] + [ms.ref[int(o):int(o) + int(n)] for o, n in zip(r_off, r_len)]
    found = []
    for c, (p, _, anchors) in enumerate(chains):
        a0 = int(first[c])
        found.append((p, len(rs) + c, [(qa, int(r_anchor[a0 + i]), g) for i, (qa, _, g) in enumerate(anchors)], rs.reads[p][1]))
    return chain_ref.ChainSet(seqs, found, True), shift


def overlaps_origin(ms: MappingSet, i: int, r_start: int, r_end: int) -> bool:
    a, b, _ = ms.origin[i]
    return r_start < b and a < r_end
