"""A pure-Python model of colinear anchor chaining ("Chaining anchors"): the fill, the picking and the output anchors of one
problem, all in integers, and generators of the problem sets the GPU tests compare AnchorChainer with. chain() is what ba_chaining_* must
report for one problem, bit for bit."""
import itertools
from collections import namedtuple

import numpy as np

Params = namedtuple("Params", "match_w drift_cost skip_cost lookback max_dist bandwidth max_chains min_score min_anchors")
NONE = -1

KNOWN_PARAMS = Params(4, 1, 0, 64, 500, 100, 3, 20, 1)
KNOWN_Q = [40, 0, 12, 30, 300, 52, 60, 90]
KNOWN_R = [8, 5, 20, 38, 45, 63, 70, 100]
KNOWN_L = [6, 10, 12, 10, 8, 12, 10, 15]
KNOWN_F = [24, 40, 85, 125, 32, 170, 189, 249]
KNOWN_PRED = [NONE, NONE, 1, 2, NONE, 3, 5, 6]
KNOWN_CHAINS = [(249, [(0, 5, 10, 1), (12, 20, 12, 2), (30, 38, 10, 3), (52, 63, 12, 5), (65, 75, 5, 6), (90, 100, 15, 7)]),
                (32, [(300, 45, 8, 4)]),
                (24, [(40, 8, 6, 0)])]
CASES = ("trimmed", "cut_at_used", "dropped_min_anchors", "tie_none", "tie_nearer")


def link(P: Params, qe_i, re_i, L_i, qe_j, re_j, f_j):
    """The value and the gain of anchor i behind anchor j, or None if j is not admissible."""
    dq, dr = qe_i - qe_j, re_i - re_j
    if not (dq > 0 and dr > 0 and dq <= P.max_dist and dr <= P.max_dist and abs(dq - dr) <= P.bandwidth):
        return None
    g = min(L_i, dq, dr)
    return f_j + P.match_w * g - P.drift_cost * abs(dq - dr) - P.skip_cost * (min(dq, dr) - g), g


def fill(P: Params, q, r, L, counts=None):
    """-> (f, pred, gain) of one problem's anchors (sorted by (re, qe)); pred is NONE or an index of the problem."""
    n = len(q)
    qe = [int(q[i]) + int(L[i]) for i in range(n)]
    re = [int(r[i]) + int(L[i]) for i in range(n)]
    f, pred, gain = [0] * n, [NONE] * n, [0] * n
    for i in range(n):
        best, p, g = P.match_w * int(L[i]), NONE, int(L[i])
        tie = None   # the last candidate that equalled the value that won in the end
        for j in range(i - 1, max(0, i - P.lookback) - 1, -1):
            vg = link(P, qe[i], re[i], int(L[i]), qe[j], re[j], f[j])
            if vg is None:
                continue
            if vg[0] > best:
                best, p, g, tie = vg[0], j, vg[1], None
            elif vg[0] == best:
                tie = "tie_none" if p == NONE else "tie_nearer"
        if tie and counts is not None:
            counts[tie] = counts.get(tie, 0) + 1
        f[i], pred[i], gain[i] = best, p, g
    return f, pred, gain


def pick(P: Params, q, r, L, f, pred, gain, counts=None):
    """-> the kept chains in the order picked: [(score, [(q, r, len, src)])]."""
    n = len(f)
    used = [False] * n
    chains = []
    for _ in range(P.max_chains):
        e = NONE
        for i in range(n):
            if not used[i] and (e == NONE or f[i] > f[e]):
                e = i
        if e == NONE or f[e] < P.min_score:
            break
        path, k = [], e
        while k != NONE and not used[k]:
            path.append(k)
            used[k] = True
            k = pred[k]
        score = f[e] if k == NONE else f[e] - f[k]
        if score >= P.min_score and len(path) >= P.min_anchors:
            path.reverse()
            out = []
            for x in path:
                g = gain[x]   # (an anchor without a predecessor has gain = L: a chain that ended at "none" starts with a whole anchor)
                out.append((int(q[x]) + int(L[x]) - g, int(r[x]) + int(L[x]) - g, g, x))
            chains.append((score, out))
            if counts is not None:
                counts["trimmed"] = counts.get("trimmed", 0) + sum(1 for x in path if gain[x] < int(L[x]))
                counts["cut_at_used"] = counts.get("cut_at_used", 0) + (k != NONE)
        elif counts is not None and score >= P.min_score:
            counts["dropped_min_anchors"] = counts.get("dropped_min_anchors", 0) + 1
    return chains


def chain(P: Params, q, r, L, counts=None):
    """One problem -> dict(f, pred, gain, chains)."""
    f, pred, gain = fill(P, q, r, L, counts)
    return dict(f=f, pred=pred, gain=gain, chains=pick(P, q, r, L, f, pred, gain, counts))


def exhaustive_best(P: Params, q, r, L):
    """The best score over every subsequence of the anchors whose consecutive members are admissible (small n only)."""
    n = len(q)
    qe = [int(q[i]) + int(L[i]) for i in range(n)]
    re = [int(r[i]) + int(L[i]) for i in range(n)]
    best = None
    for k in range(1, n + 1):
        for sub in itertools.combinations(range(n), k):
            s = P.match_w * int(L[sub[0]])
            for a, b in zip(sub, sub[1:]):
                vg = link(P, qe[b], re[b], int(L[b]), qe[a], re[a], s)
                if vg is None:
                    s = None
                    break
                s = vg[0]
            if s is not None and (best is None or s > best):
                best = s
    return best


def check_output(P: Params, q, r, L, chains):
    """What ba_chain_batch_create insists on, and what the rule promises, of one problem's chains."""
    seen = set()
    for score, anchors in chains:
        assert score >= P.min_score and len(anchors) >= P.min_anchors
        for k, (qa, ra, g, src) in enumerate(anchors):
            assert g >= 1 and src not in seen
            seen.add(src)
            assert qa + g == int(q[src]) + int(L[src]) and ra + g == int(r[src]) + int(L[src]) and g <= int(L[src])
            if k:
                pq, pr, pg, _ = anchors[k - 1]
                assert pq + pg <= qa and pr + pg <= ra, (anchors[k - 1], anchors[k])


# ------------------------------------------------------------------ problem sets
class ProblemSet:
    """Problems in the layout ba_chaining_create takes. problems: [(q, r, L)] per problem, each sorted here by (re, qe)."""

    def __init__(self, problems):
        self.problems = []
        for q, r, L in problems:
            q, r, L = (np.asarray(x, np.int64) for x in (q, r, L))
            o = np.lexsort((q + L, r + L))
            self.problems.append((q[o].astype(np.uint32), r[o].astype(np.uint32), L[o].astype(np.uint32)))
        self.anchor_first = np.concatenate([[0], np.cumsum([len(p[0]) for p in self.problems])]).astype(np.uint64)
        cat = lambda k: np.concatenate([p[k] for p in self.problems]).astype(np.uint32) if self.problems else np.zeros(0, np.uint32)
        self.q_anchor, self.r_anchor, self.anchor_len = cat(0), cat(1), cat(2)

    def __len__(self):
        return len(self.problems)

    def args(self):
        return (self.anchor_first, self.q_anchor, self.r_anchor, self.anchor_len)

    def expected(self, P: Params, counts=None):
        return [chain(P, *p, counts=counts) for p in self.problems]


def random_problem(rng, n, span=None, kmer=(6, 15), noise=0.3, step=(1, 12), indel=0.15):
    """n hits: overlapping k-mer hits along a drifting diagonal (the true chain), and `noise` of them anywhere."""
    span = span or max(200, 8 * n)
    q, r, L = [], [], []
    x, y = int(rng.integers(0, 50)), int(rng.integers(0, 50))
    for _ in range(n):
        k = int(rng.integers(kmer[0], kmer[1] + 1))
        if rng.random() < noise:
            q.append(int(rng.integers(0, span))); r.append(int(rng.integers(0, span))); L.append(k)
            continue
        q.append(x); r.append(y); L.append(k)
        d = int(rng.integers(step[0], step[1] + 1))
        x += d; y += d
        if rng.random() < indel:
            if rng.random() < 0.5:
                x += int(rng.integers(1, 8))
            else:
                y += int(rng.integers(1, 8))
    return q, r, L


def tie_problem():
    """Equal candidates, far from one another (max_dist 400). B behind A is worth exactly what B is worth alone (4 * 6 + 4 * 6 - 24 drift):
    "none" wins. E behind C and E behind D are worth the same 30 and C cannot precede D: the nearer D wins."""
    q = [1000, 1006, 2002, 2000, 2024]
    r = [1000, 1030, 2000, 2002, 2024]
    L = [6, 6, 6, 6, 6]
    return q, r, L


def far_problem(gaps=(70, 600, 1000, 30)):
    """A chain whose consecutive anchors lie gaps[k] + 1 apart in the sorted order: between two of them sit hits that end at the same
    reference position as the first (so they follow it in the order, and are admissible to nothing before the second: dr = 0 among
    themselves) and far behind the second on the query (dq < 0). The second anchor's only admissible predecessor is the first."""
    q, r, L = [], [], []
    for k, m in enumerate(gaps + (0,)):
        q.append(12 * k); r.append(15 * k); L.append(10)
        q += [5000 + 2000 * k + i for i in range(m)]; r += [15 * k] * m; L += [10] * m
    return q, r, L


def gpu_sets():
    """The problem sets of tests/test_gpu_chaining.py, by name -> (Params, ProblemSet). tests/test_chaining_ref.py asserts on the CPU that
    together they meet every case of CASES."""
    rng = np.random.default_rng(2024)
    P = Params(4, 1, 1, 64, 400, 60, 4, 24, 2)
    sizes = ProblemSet([random_problem(rng, n) for n in (0, 1, 63, 64, 65, 2, 130)] + [tie_problem()])
    big = ProblemSet([random_problem(rng, 3000, span=20000), random_problem(rng, 5), random_problem(rng, 700, noise=0.6)])
    tiny = ProblemSet([random_problem(rng, int(rng.integers(0, 9)), span=60, noise=0.2) for _ in range(2000)])
    smaller = ProblemSet([random_problem(rng, n) for n in (40, 0, 64, 7)])
    wide = ProblemSet([far_problem(), random_problem(rng, 300)])
    return dict(known=(KNOWN_PARAMS, ProblemSet([(KNOWN_Q, KNOWN_R, KNOWN_L)])),
                sizes=(P, sizes), big=(P._replace(lookback=200), big), tiny=(P._replace(min_score=16, min_anchors=1), tiny),
                smaller=(P, smaller), wide=(P._replace(lookback=1024, max_dist=20000, bandwidth=300), wide))


LOOKBACKS = (1, 63, 64, 65, 200)
WIDE_LOOKBACKS = (960, 961, 1000, 1001, 1024)   # a ring of 1024 slots; the first with 2048 (two waves per workgroup); far_problem's reach; the limit
MAX_CHAINS = (1, 8)


# ------------------------------------------------------------------ end to end: raw hits of the true anchors of a chain set
def raw_hits(cs, c, rng, band, k=8, step=3, noise=30, cells_per_noise_hit=40000):
    """Chain c of a tests/chain_ref.py set as a mapper's raw hits: every true anchor of at least k columns broken into overlapping k-mers
    (every `step` columns, and its last k), shorter ones whole, plus random off-diagonal hits -- one per `cells_per_noise_hit` cells of the
    read's matrix, at least 2 and at most `noise`, so that on a short read the noise does not outweigh the few true anchors --: more than
    `band` diagonals away from every true anchor, so that no link between a noise hit and a true one is admissible under bandwidth = band.
    -> (q, r, L, noise hits added)."""
    q, r, L = [], [], []
    diags = set()
    for qa, ra, n in cs.anchors(c):
        diags.add(qa - ra)
        if n < k:
            q.append(qa); r.append(ra); L.append(n)
            continue
        for s in sorted(set(range(0, n - k + 1, step)) | {n - k}):
            q.append(qa + s); r.append(ra + s); L.append(k)
    ql, rl = len(cs.q(c)), len(cs.r(c))
    noise = max(2, min(noise, ql * rl // cells_per_noise_hit))
    added = 0
    for _ in range(10 * noise):
        if added == noise or ql <= k or rl <= k:
            break
        a, b = int(rng.integers(0, ql - k)), int(rng.integers(0, rl - k))
        if min(abs(a - b - d) for d in diags) <= band:
            continue
        q.append(a); r.append(b); L.append(k); added += 1
    return q, r, L, added


def true_positions(cs, c):
    return {(qa + x, ra + x) for qa, ra, n in cs.anchors(c) for x in range(n)}


E2E_PARAMS = Params(4, 2, 0, 64, 400, 50, 2, 32, 1)


def e2e_problems(cs, seed=5):
    """-> (ProblemSet, noise hits added): the raw hits of every chain of cs."""
    rng = np.random.default_rng(seed)
    hits = [raw_hits(cs, c, rng, E2E_PARAMS.bandwidth) for c in range(len(cs))]
    return ProblemSet([h[:3] for h in hits]), sum(h[3] for h in hits)
