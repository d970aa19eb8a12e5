"""Seed-and-extend batches on the MI355X: every field of every seed against a composite built here from the oracle -- both sides aligned
on host-reversed / host-reverse-complemented slices, the seed scored and the CIGARs spliced in Python -- and every traced result
re-scored by verify.check_cigar over q[q_start:q_end] / r[r_start:r_end]."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth, verify

pytestmark = pytest.mark.gpu

COMP = bytes.maketrans(b"ACGT", b"TGCA")
OPS = {"M": 1, "=": 2, "X": 3, "I": 4, "D": 5}


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


class SeedSet:
    def __init__(self, seqs, q_idx, r_idx, q_seed, r_seed, seed_len, strand=None):
        lens = [len(s) for s in seqs]
        off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        self.seqs = seqs
        self.pool = np.frombuffer(b"".join(seqs), dtype=np.uint8) if seqs else np.zeros(0, np.uint8)
        self.q_off, self.q_len = off[q_idx], np.array(lens, np.uint32)[q_idx]
        self.r_off, self.r_len = off[r_idx], np.array(lens, np.uint32)[r_idx]
        self.q_idx, self.r_idx = list(q_idx), list(r_idx)
        self.q_seed, self.r_seed = np.array(q_seed, np.uint32), np.array(r_seed, np.uint32)
        self.seed_len = np.array(seed_len, np.uint32)
        self.strand = None if strand is None else np.array(strand, np.uint8)

    def __len__(self):
        return len(self.q_seed)

    def args(self):
        return (self.pool, self.q_off, self.q_len, self.r_off, self.r_len, self.q_seed, self.r_seed, self.seed_len)

    def q(self, p):
        b = self.seqs[self.q_idx[p]]
        return revcomp(b) if self.strand is not None and self.strand[p] else b

    def r(self, p):
        return self.seqs[self.r_idx[p]]


def composite(oracle, m, gaps, size, x_drop, mode, ss, p):
    """The expected result of seed p: the oracle on both sides, the seed scored and the runs spliced here."""
    trace, eq = bool(mode & 1), bool(mode & 32)
    omode = ("trace", "x_drop") if trace else ("x_drop",)
    q, r = ss.q(p), ss.r(p)
    s, t, L = int(ss.q_seed[p]), int(ss.r_seed[p]), int(ss.seed_len[p])
    conv = m.convert_char
    qs, rs = [conv(c) for c in q[s:s + L].upper()], [conv(c) for c in r[t:t + L].upper()]

    def side(a, b):
        if not a or not b:
            return dict(score=0, query_idx=0, reference_idx=0, cells=0, cigar="")
        return oracle.align(m, a, b, gaps, size, x_drop, omode, cigar_eq=eq)

    left = side(q[:s][::-1], r[:t][::-1])
    right = side(q[s + L:], r[t + L:])
    seed_score = sum(m.get(a, b) for a, b in zip(q[s:s + L].upper(), r[t:t + L].upper()))
    exp = dict(score=left["score"] + seed_score + right["score"], left_score=left["score"], right_score=right["score"],
               q_start=s - left["query_idx"], r_start=t - left["reference_idx"], q_end=s + L + right["query_idx"],
               r_end=t + L + right["reference_idx"], cells=left["cells"] + right["cells"], status=0)
    if trace:
        seed = [[1, (2 if a == b else 3) if eq else 1] for a, b in zip(qs, rs)]
        runs = []
        for n, op in parse(left["cigar"])[::-1] + seed + parse(right["cigar"]):
            if runs and runs[-1][1] == op:
                runs[-1][0] += n
            else:
                runs.append([n, op])
        exp["runs"] = [n << 4 | op for n, op in runs]
    return exp


FIELDS = ("score", "left_score", "right_score", "q_start", "r_start", "q_end", "r_end", "cells", "status")


def check(hip, oracle, m, gaps, size, x_drop, mode, ss, eb=None):
    if eb is None:
        eb = hip.ExtendBatchAligner(m, gaps, size, x_drop, mode, *ss.args(), strand=ss.strand)
    eb.run()
    res = eb.results()
    runs = off = None
    if mode & 1:
        runs, off = eb.cigars(res["cigar_len"])
    with ThreadPoolExecutor(max_workers=os.cpu_count() or 4) as ex:
        exps = list(ex.map(lambda p: composite(oracle, m, gaps, size, x_drop, mode, ss, p), range(len(ss))))
    for p, exp in enumerate(exps):
        got = {k: int(res[k][p]) for k in FIELDS}
        assert got == {k: exp[k] for k in FIELDS}, (p, got, exp)
        if mode & 1:
            mine = [int(x) for x in runs[int(off[p]):int(off[p + 1])]]
            assert mine == exp["runs"], (p, hip.runs_to_string(mine), hip.runs_to_string(exp["runs"]))
            q, r = ss.q(p), ss.r(p)
            qa, ra = q[got["q_start"]:got["q_end"]], r[got["r_start"]:got["r_end"]]
            verify.check_cigar(runs[int(off[p]):int(off[p + 1])], qa, ra, m, gaps, got["score"], len(qa), len(ra), what=f"seed {p}")
        else:
            assert int(res["cigar_len"][p]) == 0
    eb.close()
    return res


def dna_seeds(rng, n, lo=200, hi=20000, minus=False, random_frac=0.1):
    """Reads of log-uniform length with mutations, indels and random flanks around a reference segment; one seed per read at a true shared
    position (an exact 15..31-mer), or, for random_frac of them, at random positions. minus: half the reads are reverse complements."""
    seqs, qi, ri, qs, rs, sl, st = [], [], [], [], [], [], []
    for p in range(n):
        rl = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
        ref = synth.rand_str(rng, rl, synth.DNA)
        L = int(rng.integers(15, 32))
        t = int(rng.integers(0, rl - L + 1))
        left = synth.mutate(rng, ref[:t], max(1, t // 25), synth.DNA)
        right = synth.mutate(rng, ref[t + L:], max(1, (rl - t - L) // 25), synth.DNA)
        fl, fr = synth.rand_str(rng, int(rng.integers(0, 200)), synth.DNA), synth.rand_str(rng, int(rng.integers(0, 200)), synth.DNA)
        read = np.concatenate([fl, left, ref[t:t + L], right, fr])
        s = len(fl) + len(left)
        if rng.random() < random_frac:
            s, t = int(rng.integers(0, len(read) - L + 1)), int(rng.integers(0, rl - L + 1))
        strand = 1 if minus and rng.random() < 0.5 else 0
        rb = read.tobytes()
        if strand:   # the caller holds the read as sequenced: the reverse complement of the reference's strand
            rb = revcomp(rb)
        if rng.random() < 0.2:
            rb = rb.lower()
        seqs += [rb, ref.tobytes()]
        qi.append(2 * p); ri.append(2 * p + 1); qs.append(s); rs.append(t); sl.append(L); st.append(strand)
    return SeedSet(seqs, qi, ri, qs, rs, sl, st if minus else None)


NUC = S.NucMatrix.new_simple(2, -3)
DNA_GAPS = (-5, -1)


@pytest.mark.parametrize("size", [(32, 256), (128, 1024)])
@pytest.mark.parametrize("mode", ["X_DROP", "TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_dna_seeds(devlib, monkeypatch, oracle, size, mode):
    """32..256 carries the sides through k_small, 128..1024 through k_multi (forced: a few hundred seeds are below their batch sizes)."""
    hip = devlib
    monkeypatch.setenv("BA_FORCE_SMALL" if size[0] == 32 else "BA_FORCE_MULTI", "1")
    flags = 0
    for f in mode.split("|"):
        flags |= getattr(hip, f)
    ss = dna_seeds(np.random.default_rng(zlib.crc32(f"{size}{mode}".encode())), 300)
    check(hip, oracle, NUC, DNA_GAPS, size, 100, flags, ss)


@pytest.mark.parametrize("mode", ["X_DROP", "TRACE|X_DROP|CIGAR_EQ"])
def test_minus_strand(hip, oracle, mode):
    flags = 0
    for f in mode.split("|"):
        flags |= getattr(hip, f)
    ss = dna_seeds(np.random.default_rng(11), 300, minus=True)
    assert ss.strand.sum() > 50
    check(hip, oracle, NUC, DNA_GAPS, (32, 256), 100, flags, ss)


@pytest.mark.parametrize("trace", [False, True])
def test_protein(hip, oracle, trace):
    """x_drop_accuracy.rs in both directions: a protein whose flanks diverge around a conserved core holding the seed."""
    rng = np.random.default_rng(5)
    seqs, qs, rs, sl = [], [], [], []
    for p in range(200):
        core = synth.rand_str(rng, int(rng.integers(100, 800)), synth.AMINO)
        mq = synth.mutate(rng, core, len(core) // 10, synth.AMINO)
        fq = [synth.rand_str(rng, int(rng.integers(0, 300)), synth.AMINO) for _ in range(2)]
        fr = [synth.rand_str(rng, int(rng.integers(0, 300)), synth.AMINO) for _ in range(2)]
        q = np.concatenate([fq[0], mq, fq[1]]).tobytes()
        r = np.concatenate([fr[0], core, fr[1]]).tobytes()
        L = int(rng.integers(4, 12))
        a = int(rng.integers(0, min(len(mq), len(core)) - L))
        seqs += [q, r]
        qs.append(min(len(fq[0]) + a, len(q) - L)); rs.append(len(fr[0]) + a); sl.append(L)
    ss = SeedSet(seqs, list(range(0, 400, 2)), list(range(1, 400, 2)), qs, rs, sl)
    mode = hip.X_DROP | (hip.TRACE if trace else 0)
    check(hip, oracle, S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, mode, ss)


def edge_set():
    a = b"ACGTTGCAAGGCTTACGATCGATCGGATCCA" * 3
    b = a[:40] + b"T" + a[41:]
    seqs = [a, b, b"ACGTAC", b"ACGTAC"]
    # (query, reference, q_seed, r_seed, seed_len)
    cases = [(0, 1, 0, 0, 10),                 # empty left side
             (0, 1, len(a) - 8, len(b) - 8, 8),   # empty right side
             (2, 3, 0, 0, 6),                  # both sides empty: the seed covers both sequences
             (0, 1, 0, 0, len(a)),             # a seed covering a whole sequence (both sides empty)
             (0, 2, 0, 2, 4),                  # left: query empty, reference not; right: reference empty
             (2, 0, 3, 20, 3),                 # right: query empty
             (0, 1, 30, 30, 12),               # ordinary
             (0, 1, 30, 60, 5)]                # a seed at unrelated positions
    return SeedSet(seqs, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])


@pytest.mark.parametrize("mode", ["TRACE|X_DROP", "TRACE|X_DROP|CIGAR_EQ", "X_DROP"])
def test_seeds_at_the_edges(hip, oracle, mode):
    flags = 0
    for f in mode.split("|"):
        flags |= getattr(hip, f)
    check(hip, oracle, NUC, DNA_GAPS, (32, 256), 20, flags, edge_set())


def test_every_side_empty(hip, oracle):
    """A set without a side to align launches no fill: results are the seeds alone."""
    ss = SeedSet([b"ACGTAC", b"ACCTAC", b"GGG"], [0, 2], [1, 2], [0, 0], [0, 0], [6, 3])
    for mode in (hip.TRACE | hip.X_DROP | hip.CIGAR_EQ, hip.X_DROP):
        res = check(hip, oracle, NUC, DNA_GAPS, (32, 256), 20, mode, ss)
        assert list(res["score"]) == [2 * 5 - 3, 6] and not res["cells"].any()


def test_long_reads(hip, oracle):
    """30 kbp reads at 128..4096: the 2048-cell class bet and its re-runs inside an extension batch."""
    ss = dna_seeds(np.random.default_rng(3), 300, lo=28000, hi=32000)
    check(hip, oracle, NUC, DNA_GAPS, (128, 4096), 100, hip.TRACE | hip.X_DROP, ss)


def test_reload_equals_fresh(hip, oracle):
    a = dna_seeds(np.random.default_rng(21), 400, lo=500, hi=8000, minus=True)
    b = dna_seeds(np.random.default_rng(22), 300, lo=400, hi=6000, minus=True)
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    eb = hip.ExtendBatchAligner(NUC, DNA_GAPS, (32, 256), 100, mode, *a.args(), strand=a.strand)
    eb.run()
    eb.reload(*b.args(), strand=b.strand)
    eb.run()
    got = eb.results()
    runs, off = eb.cigars(got["cigar_len"])
    fresh = hip.ExtendBatchAligner(NUC, DNA_GAPS, (32, 256), 100, mode, *b.args(), strand=b.strand)
    fresh.run()
    want = fresh.results()
    runs2, off2 = fresh.cigars(want["cigar_len"])
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(runs, runs2) and np.array_equal(off, off2)
    fresh.close()
    check(hip, oracle, NUC, DNA_GAPS, (32, 256), 100, mode, b, eb=eb)
