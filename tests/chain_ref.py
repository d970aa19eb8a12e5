"""A pure-Python model of anchor-chain batches ("Anchor chains") and a generator of chain sets. Given a function that aligns
one piece -- the oracle --, chain_result() gives what ChainBatchAligner must report for a chain: the left end reversed, anchor 0, gap 0,
anchor 1, ..., the last anchor, the right end, merged at every join."""
import numpy as np

from block_aligner_amd import synth

COMP = bytes.maketrans(b"ACGT", b"TGCA")
OPS = {"M": 1, "=": 2, "X": 3, "I": 4, "D": 5}
FIELDS = ("score", "left_score", "right_score", "q_start", "r_start", "q_end", "r_end", "cells", "status")


def revcomp(b: bytes) -> bytes:
    return b.upper().translate(COMP)[::-1]


def parse(cigar: str):
    out, num = [], ""
    for c in cigar:
        if c.isdigit():
            num += c
        else:
            out.append([int(num), OPS[c]])
            num = ""
    return out


def oracle_piece(oracle, m, gaps, size, x_drop, trace, eq):
    """The piece function over the oracle: piece(kind, a, b) with kind 'end' (X-drop) or 'gap' (global), both sequences non-empty."""
    t = ("trace",) if trace else ()

    def piece(kind, a, b):
        if kind == "gap":
            return oracle.align(m, a, b, gaps, size, 0, t, cigar_eq=eq)
        return oracle.align(m, a, b, gaps, size, x_drop, t + ("x_drop",), cigar_eq=eq)
    return piece


def chain_result(piece, m, gaps, q: bytes, r: bytes, anchors, trace: bool, eq: bool, counts=None):
    """The expected result of one chain. q, r: the oriented query and the reference; anchors: [(q_anchor, r_anchor, anchor_len)], colinear.
    -> dict of FIELDS and, with trace, `runs` (len << 4 | op). counts (optional dict): what the chain exercised is added to it."""
    elements = []   # per element its runs [[len, op]]; score, cells are summed as we go
    score = cells = 0
    empty = dict(score=0, query_idx=0, reference_idx=0, cells=0, cigar="")
    s, t, _ = anchors[0]
    left = piece("end", q[:s][::-1], r[:t][::-1]) if s and t else empty
    elements.append(parse(left["cigar"])[::-1])
    kind_of = ["end"]
    stats = dict(gap_none=0, gap_query_only=0, gap_reference_only=0, gap_aligned=0)
    for k, (qa, ra, L) in enumerate(anchors):
        qs, rs = q[qa:qa + L].upper(), r[ra:ra + L].upper()
        if getattr(m, "KIND", 1) == 2:
            qs, rs = q[qa:qa + L], r[ra:ra + L]
        assert len(qs) == L and len(rs) == L, "anchor past the end"
        score += sum(m.get(a, b) for a, b in zip(qs, rs))
        runs = []
        for a, b in zip(qs, rs):
            op = (2 if a == b else 3) if eq else 1
            if runs and runs[-1][1] == op:
                runs[-1][0] += 1
            else:
                runs.append([1, op])
        elements.append(runs); kind_of.append("anchor")
        if k + 1 < len(anchors):
            nq, nr, _ = anchors[k + 1]
            assert qa + L <= nq and ra + L <= nr, "anchors overlap or are out of order"
            gq, gr = q[qa + L:nq], r[ra + L:nr]
            if gq and gr:
                g = piece("gap", gq, gr)
                assert (g["query_idx"], g["reference_idx"]) == (len(gq), len(gr)), "a global piece ends at its corner"
                score += g["score"]; cells += g["cells"]
                elements.append(parse(g["cigar"])); stats["gap_aligned"] += 1
            elif gq or gr:
                d = len(gq) + len(gr)
                score += gaps[0] + (d - 1) * gaps[1]
                elements.append([[d, 4 if gq else 5]])
                stats["gap_query_only" if gq else "gap_reference_only"] += 1
            else:
                elements.append([]); stats["gap_none"] += 1
            kind_of.append("gap")
    qe, re_ = anchors[-1][0] + anchors[-1][2], anchors[-1][1] + anchors[-1][2]
    right = piece("end", q[qe:], r[re_:]) if len(q) > qe and len(r) > re_ else empty
    elements.append(parse(right["cigar"])); kind_of.append("end")
    out = dict(score=score + left["score"] + right["score"], left_score=left["score"], right_score=right["score"],
               q_start=s - left["query_idx"], r_start=t - left["reference_idx"], q_end=qe + right["query_idx"], r_end=re_ + right["reference_idx"],
               cells=cells + left["cells"] + right["cells"], status=0)
    if trace:
        runs, members = [], []   # members: the elements a merged run came from
        merges = gap_merges = 0
        for e, el in enumerate(elements):
            for n, op in el:
                if runs and runs[-1][1] == op:
                    runs[-1][0] += n
                    assert members[-1][-1] != e, "an element's own runs alternate"
                    gap_merges += kind_of[e] == "gap" and kind_of[members[-1][-1]] == "gap"
                    members[-1].append(e); merges += 1
                else:
                    runs.append([n, op]); members.append([e])
        assert gap_merges == 0   # every gap is separated from the next by an anchor: two gap runs never merge
        out["runs"] = [n << 4 | op for n, op in runs]
        stats["merges"] = merges
        stats["wide_groups"] = sum(1 for mem in members if len(mem) >= 3)
    stats["chains_130"] = int(len(elements) >= 130)
    if counts is not None:
        for k, v in stats.items():
            counts[k] = counts.get(k, 0) + v
    return out


class ChainSet:
    """Chains over a pool of sequences, in the layout ChainBatchAligner takes. chains: [(query index, reference index, [(qa, ra, L)], strand)]."""

    def __init__(self, seqs, chains, with_strand=False):
        lens = [len(s) for s in seqs]
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        self.seqs, self.chains = seqs, chains
        self.pool = np.frombuffer(b"".join(seqs) + bytes(8), dtype=np.uint8)
        qi, ri = [c[0] for c in chains], [c[1] for c in chains]
        self.q_off, self.q_len = off[qi], np.array(lens, np.uint32)[qi]
        self.r_off, self.r_len = off[ri], np.array(lens, np.uint32)[ri]
        self.anchor_first = np.concatenate([[0], np.cumsum([len(c[2]) for c in chains])]).astype(np.uint64)
        flat = [a for c in chains for a in c[2]]
        self.q_anchor = np.array([a[0] for a in flat], np.uint32)
        self.r_anchor = np.array([a[1] for a in flat], np.uint32)
        self.anchor_len = np.array([a[2] for a in flat], np.uint32)
        self.strand = np.array([c[3] for c in chains], np.uint8) if with_strand else None

    def __len__(self):
        return len(self.chains)

    def args(self):
        return (self.pool, self.q_off, self.q_len, self.r_off, self.r_len, self.anchor_first, self.q_anchor, self.r_anchor, self.anchor_len)

    def q(self, c):
        b = self.seqs[self.chains[c][0]]
        return revcomp(b) if self.chains[c][3] else b

    def r(self, c):
        return self.seqs[self.chains[c][1]]

    def anchors(self, c):
        return self.chains[c][2]

    def subset(self, idx):
        return ChainSet(self.seqs, [self.chains[c] for c in idx], self.strand is not None)

    def first_anchor_seeds(self):
        """Every chain cut down to its first anchor (K = 1): a seed set in ExtendBatchAligner's layout."""
        return ChainSet(self.seqs, [(c[0], c[1], c[2][:1], c[3]) for c in self.chains], self.strand is not None)


def expected(piece, m, gaps, cs: ChainSet, trace, eq, counts=None):
    return [chain_result(piece, m, gaps, cs.q(c), cs.r(c), cs.anchors(c), trace, eq, counts) for c in range(len(cs))]


def make_chain(rng, ref_len, alphabet=synth.DNA, spacing=(20, 150), anchor=(8, 24), edit_div=12, flank=60, p_adjacent=0.15, p_query_only=0.1,
               p_reference_only=0.1, p_mismatch_anchor=0.15):
    """One read derived from a random reference, with its anchors at true shared positions -> (read, reference, anchors). Between two anchors
    the read holds a mutated copy of the reference's stretch, or (p_adjacent) nothing on either side, or (p_query_only) inserted bytes only,
    or (p_reference_only) nothing where the reference has bytes; an anchor is an exact copy or (p_mismatch_anchor) has one substitution."""
    ref = synth.rand_str(rng, ref_len, alphabet)
    read = [synth.rand_str(rng, int(rng.integers(0, flank + 1)), alphabet)]
    rlen = len(read[0])
    t = int(rng.integers(0, max(1, min(flank, ref_len // 4))))
    head = synth.mutate(rng, ref[:t], max(1, t // edit_div), alphabet)
    read.append(head); rlen += len(head)
    anchors = []
    while True:
        L = int(rng.integers(anchor[0], anchor[1] + 1))
        if t + L > ref_len:
            break
        a = ref[t:t + L].copy()
        if L >= 3 and rng.random() < p_mismatch_anchor:
            k = int(rng.integers(1, L - 1))
            a[k] = alphabet[(int(np.nonzero(alphabet == a[k])[0][0]) + 1) % len(alphabet)]
        anchors.append((rlen, t, L))
        read.append(a); rlen += L; t += L
        u, d = rng.random(), int(rng.integers(spacing[0], spacing[1] + 1))
        if u < p_adjacent:
            continue
        if u < p_adjacent + p_query_only:
            ins = synth.rand_str(rng, int(rng.integers(1, 12)), alphabet)
            read.append(ins); rlen += len(ins)
            continue
        if t + d > ref_len:
            break
        if u < p_adjacent + p_query_only + p_reference_only:
            t += int(rng.integers(1, 12))
            continue
        mid = synth.mutate(rng, ref[t:t + d], max(1, d // edit_div), alphabet)
        if len(mid) == 0:
            mid = synth.rand_str(rng, 1, alphabet)
        read.append(mid); rlen += len(mid); t += d
    while anchors and anchors[-1][1] + anchors[-1][2] > ref_len:
        anchors.pop()
    tail = synth.mutate(rng, ref[anchors[-1][1] + anchors[-1][2]:], max(1, (ref_len - t) // edit_div), alphabet) if anchors else ref[:0]
    read.append(tail)
    read.append(synth.rand_str(rng, int(rng.integers(0, flank + 1)), alphabet))
    return np.concatenate(read).tobytes(), ref.tobytes(), anchors


def make_set(rng, n, lo=200, hi=3000, alphabet=synth.DNA, minus=False, lower=True, **kw) -> ChainSet:
    """n chains over reads of lo .. hi bases (log-uniform). minus: half the reads are held as sequenced from the other strand; lower: a fifth
    of the reads are lower case."""
    seqs, chains = [], []
    while len(chains) < n:
        ref_len = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        read, ref, anchors = make_chain(rng, ref_len, alphabet, **kw)
        if not anchors:
            continue
        strand = 1 if minus and rng.random() < 0.5 else 0
        if strand:
            read = revcomp(read)
        if lower and rng.random() < 0.2:
            read = read.lower()
        chains.append((len(seqs), len(seqs) + 1, anchors, strand))
        seqs += [read, ref]
    return ChainSet(seqs, chains, minus)


def without_ends(src: ChainSet, n=None) -> ChainSet:
    """The chains of src (the first n) over trimmed sequences: the query starts with the first anchor and ends with the last one (the
    reference goes on behind it), so no chain has an end to extend. Plus strand only."""
    seqs, chains = [], []
    for c in range(len(src) if n is None else n):
        assert not src.chains[c][3]
        an = src.anchors(c)
        (s, t, _), (ls, _, ll) = an[0], an[-1]
        chains.append((len(seqs), len(seqs) + 1, [(a - s, b - t, k) for a, b, k in an], 0))
        seqs += [src.q(c)[s:ls + ll], src.r(c)[t:]]
    return ChainSet(seqs, chains)


def dna_sets():
    """The DNA sets of the GPU parity tests, by name (tests/test_chain_ref.py asserts on the CPU that they meet every case of the splice)."""
    return dict(mixed=make_set(np.random.default_rng(101), 150),
                dense=make_set(np.random.default_rng(102), 40, lo=2000, hi=3000, spacing=(4, 40), anchor=(6, 16)),
                minus=make_set(np.random.default_rng(103), 120, minus=True))


def collapse_chain(n_anchors=130, L=5, flank=40, seed=1):
    """One chain of n_anchors adjacent exact-match anchors with nothing between them, unrelated flanks on both sides."""
    rng = np.random.default_rng(seed)
    core = synth.rand_str(rng, n_anchors * L, synth.DNA).tobytes()
    fl = [synth.rand_str(rng, flank, synth.DNA).tobytes() for _ in range(4)]
    anchors = [(flank + k * L, flank + k * L, L) for k in range(n_anchors)]
    return ChainSet([fl[0] + core + fl[1], fl[2] + core + fl[3]], [(0, 1, anchors, 0)])
