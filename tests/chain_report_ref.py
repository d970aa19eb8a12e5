"""The statistics of a chain as the device combines them (k_stats_chain, ba_stats.hip), stated in Python: one tests/test_gpu_stats.py::
ref_stats record per element of the chain -- the left end, anchor 0, gap 0, ..., the right end --, added up and maximised. And the chain
sets the report's tests share (tests/test_chain_report_ref.py asserts on the CPU what they cover; tests/test_gpu_chain_report.py runs them)."""
import numpy as np

from block_aligner_amd import scores as S, synth
from tests import chain_ref as R
from tests.test_gpu_stats import FIELDS, ref_stats

NUC = S.NucMatrix.new_simple(2, -3)
DNA = dict(m=NUC, gaps=(-5, -1), size=(32, 256), x_drop=100)
PROTEIN = dict(m=S.static_matrix("BLOSUM62"), gaps=(-11, -1), size=(32, 256), x_drop=50)
BYTES = dict(m=S.ByteMatrix.new_simple(3, -2), gaps=(-4, -2), size=(32, 256), x_drop=40)
SUMMED = ("columns", "matches", "mismatches", "positives", "ins", "del", "gap_opens", "path_score")
LONGEST = ("longest_ins", "longest_del")


def element_records(piece, m, gaps, q: bytes, r: bytes, anchors, eq: bool, counts=None):
    """-> ([(kind, record)] in path order, (q_start, r_start)): every element's own ref_stats record over its own slices."""
    def rec(runs, a, b, qi, ri):
        return ref_stats([n << 4 | op for n, op in runs], a, b, m, gaps, qi, ri)

    def count(k):
        if counts is not None:
            counts[k] = counts.get(k, 0) + 1

    out = []
    s, t, _ = anchors[0]
    lq = lr = 0
    if s and t:
        a, b = q[:s][::-1], r[:t][::-1]
        left = piece("end", a, b)
        lq, lr = left["query_idx"], left["reference_idx"]
        out.append(("end", rec(R.parse(left["cigar"]), a, b, lq, lr)))   # (the runs of the reversed prefixes: the counts are those of the reversal)
        count("left_end")
    else:
        count("no_left_end")
    for k, (qa, ra, L) in enumerate(anchors):
        a, b = q[qa:qa + L], r[ra:ra + L]
        up = (lambda x: x) if getattr(m, "KIND", 1) == 2 else bytes.upper
        cols = [(2 if x == y else 3) if eq else 1 for x, y in zip(up(a), up(b))]
        runs = []
        for op in cols:
            if runs and runs[-1][1] == op:
                runs[-1][0] += 1
            else:
                runs.append([1, op])
        out.append(("anchor", rec(runs, a, b, L, L)))
        if up(a) != up(b):
            count("mismatching_anchor")
        if k + 1 < len(anchors):
            nq, nr, _ = anchors[k + 1]
            gq, gr = q[qa + L:nq], r[ra + L:nr]
            if gq and gr:
                g = piece("gap", gq, gr)
                out.append(("gap", rec(R.parse(g["cigar"]), gq, gr, len(gq), len(gr))))
                count("gap_aligned")
            elif gq or gr:
                d = len(gq) + len(gr)
                out.append(("gap", rec([[d, 4 if gq else 5]], gq, gr, len(gq), len(gr))))
                count("gap_query_only" if gq else "gap_reference_only")
            else:
                count("gap_none")
    qe, re_ = anchors[-1][0] + anchors[-1][2], anchors[-1][1] + anchors[-1][2]
    if len(q) > qe and len(r) > re_:
        right = piece("end", q[qe:], r[re_:])
        out.append(("end", rec(R.parse(right["cigar"]), q[qe:], r[re_:], right["query_idx"], right["reference_idx"])))
        count("right_end")
    else:
        count("no_right_end")
    return out, (s - lq, t - lr)


def combine(records, start):
    """The combine rule: counts add, the longest gaps take the maximum, the start is the first anchor's less what the left end consumed."""
    rec = dict.fromkeys(FIELDS, 0)
    for _, x in records:
        for k in SUMMED:
            rec[k] += x[k]
        for k in LONGEST:
            rec[k] = max(rec[k], x[k])
    rec["q_start"], rec["r_start"] = start
    return rec


def whole_record(exp, m, gaps, q: bytes, r: bytes):
    """The record the report must give: ref_stats of the chain's spliced runs over the oriented query and the reference."""
    return ref_stats(exp["runs"], q, r, m, gaps, exp["q_end"], exp["r_end"], exp["status"])


def protein_set():
    return R.make_set(np.random.default_rng(7), 40, lo=200, hi=1200, alphabet=synth.AMINO, spacing=(10, 80), anchor=(4, 12), edit_div=6)


def bytes_set():
    """(A ByteMatrix scores its padding as a mismatch, so an X-drop end may stop in the padding, which the oracle's traceback refuses: the
    chains of this set have no ends -- tests/test_gpu_chain.py::test_bytes.)"""
    return R.without_ends(R.make_set(np.random.default_rng(8), 40, lo=200, hi=1200, alphabet=np.arange(250, 256, dtype=np.uint8), lower=False))


def no_aligned_gap_set():
    return R.make_set(np.random.default_rng(9), 60, lo=200, hi=800, p_adjacent=0.4, p_query_only=0.3, p_reference_only=0.31)


BOUNDARY_K = (1, 2, 31, 32, 33, 63, 64, 65, 130)


def chain_of(K: int, seed: int):
    """One chain of exactly K anchors with mixed gaps, a short tail behind the last one -> (read, reference, anchors)."""
    rng = np.random.default_rng(seed)
    while True:
        read, ref, anchors = R.make_chain(rng, 60 * K + 300, spacing=(4, 40), anchor=(6, 16), p_adjacent=0.2, p_query_only=0.15, p_reference_only=0.15)
        if len(anchors) >= K:
            break
    anchors = anchors[:K]
    qa, ra, L = anchors[-1]
    return read[:qa + L + 30], ref[:ra + L + 25], anchors


def long_anchor_chain(L=300, flank=40, seed=3):
    """One chain of a single anchor of L columns holding three mismatches: the anchor's columns go over the whole wave."""
    rng = np.random.default_rng(seed)
    core = synth.rand_str(rng, L, synth.DNA)
    read = core.copy()
    for k in (1, 150, 298):
        read[k] = synth.DNA[(int(np.nonzero(synth.DNA == core[k])[0][0]) + 1) % 4]
    fl = [synth.rand_str(rng, flank, synth.DNA).tobytes() for _ in range(4)]
    return fl[0] + read.tobytes() + fl[1], fl[2] + core.tobytes() + fl[3], [(flank, flank, L)]


def boundary_set():
    """One chain each for K in BOUNDARY_K (2 K + 1 elements: around the edges of the wave's chunks of 64), 130 adjacent exact anchors, and
    the long anchor."""
    seqs, chains = [], []
    for read, ref, anchors in [chain_of(K, 40 + K) for K in BOUNDARY_K] + [long_anchor_chain()]:
        chains.append((len(seqs), len(seqs) + 1, anchors, 0))
        seqs += [read, ref]
    col = R.collapse_chain(130)
    chains.append((len(seqs), len(seqs) + 1, col.anchors(0), 0))
    seqs += list(col.seqs)
    return R.ChainSet(seqs, chains)


def wide_gap_chain(eq: bool, seed=5):
    """Three anchors, two gaps of 600 reference bases; the read differs every few bases -- by a substitution (eq: = and X runs alternate) or
    by a missing base (M and D runs alternate) --, so that each gap piece has more than 64 runs (the generator of tests/test_gpu_chain.py)."""
    rng = np.random.default_rng(seed)
    anchors, read, ref, L = [], [], [], 20
    for k in range(3):
        a = synth.rand_str(rng, L, synth.DNA)
        anchors.append((sum(map(len, read)), sum(map(len, ref)), L))
        read.append(a); ref.append(a)
        if k < 2:
            g = synth.rand_str(rng, 600, synth.DNA)
            ref.append(g)
            if eq:
                h = g.copy()
                h[3::7] = np.frombuffer(g.tobytes().translate(bytes.maketrans(b"ACGT", b"CGTA")), np.uint8)[3::7]
                read.append(h)
            else:
                read.append(np.delete(g, np.arange(4, 600, 8)))
    return R.ChainSet([np.concatenate(read).tobytes(), np.concatenate(ref).tobytes()], [(0, 1, anchors, 0)])
