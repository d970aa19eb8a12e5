"""Models of an index over several reference sequences ("Several sequences"), in integers, on top of tests/index_ref.py,
tests/seeding_ref.py and tests/chaining_ref.py: the index's entries, the hits of a read against them, the fill and the chains bounded by a
sequence table, the candidate windows inside one sequence and the way back from the index's frame. Each is what the library must report,
bit for bit. Also the problem sets and the read set that the CPU and the GPU tests share."""
import numpy as np

from tests import chaining_ref as C, index_ref as X, seeding_ref as S

MAX_SEQS = 1 << 20
MAX_TOTAL = 0x7fffffff - 16   # ba::SEEDING_MAX_LEN: the sequences together stay below it


def seq_start(seqs):
    """Where the sequences start when laid end to end, and where the last one ends: len(seqs) + 1 integers."""
    out = [0]
    for s in seqs:
        out.append(out[-1] + len(s))
    return out


def seq_of(start, pos: int) -> int:
    """The last non-empty sequence that starts at or before pos (0 when every sequence is empty)."""
    best = 0
    for s in range(len(start) - 1):
        if start[s + 1] > start[s] and start[s] <= pos:
            best = s
    return best


def sketch_multi(seqs, k: int, w: int):
    """-> (pos, code) of every sequence's own sketch, positions in the index's frame, in position order."""
    pos, code = [np.zeros(0, np.uint32)], [np.zeros(0, np.uint32)]
    for s, at in zip(seqs, seq_start(seqs)):
        p, c = S.sketch(bytes(s), k, w)
        pos.append((p.astype(np.int64) + at).astype(np.uint32))
        code.append(c)
    return np.concatenate(pos), np.concatenate(code)


def entries_multi(seqs, k: int, w: int):
    """-> (code, pos) of the index, ascending by (code, pos), and longest_run: the union of index_ref.entries per sequence, shifted."""
    code, pos = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)]
    for s, at in zip(seqs, seq_start(seqs)):
        c, p, _ = X.entries(s, k, w)
        code.append(c.astype(np.uint64))
        pos.append(p.astype(np.uint64) + np.uint64(at))
    key = np.sort(np.concatenate(code) << np.uint64(32) | np.concatenate(pos))
    code = (key >> np.uint64(32)).astype(np.uint32)
    longest = int(np.unique(code, return_counts=True)[1].max()) if len(code) else 0
    return code, (key & np.uint64(S.MASK)).astype(np.uint32), longest


def hits_multi(q: bytes, seqs, P: X.Params, strand: int = 0):
    """The hits rule over the union sketch: a query code over max_occ gives nothing, and neither does a reference entry whose code occurs
    more than max_ref_occ times in all sequences together -> dict(q_pos, q_code, q_hit, r_hit), the hits by (r_hit, q_hit)."""
    qp, qc = S.sketch(S.oriented(q, strand), P.k, P.w)
    rp, rc = sketch_multi(seqs, P.k, P.w)
    q_at = {}
    for i, c in zip(qp.tolist(), qc.tolist()):
        q_at.setdefault(c, []).append(i)
    codes, counts = np.unique(rc, return_counts=True)
    occ = dict(zip(codes.tolist(), counts.tolist()))
    q_hit, r_hit = [], []
    for j, c in zip(rp.tolist(), rc.tolist()):
        m = q_at.get(c, [])
        if 1 <= len(m) <= P.max_occ and occ[c] <= P.max_ref_occ:
            q_hit += m
            r_hit += [j] * len(m)
    return dict(q_pos=qp, q_code=qc, q_hit=np.array(q_hit, np.uint32), r_hit=np.array(r_hit, np.uint32))


def fill_bounded(P: C.Params, q, r, L, start):
    """chaining_ref.fill with one more condition on a predecessor j of anchor i: re_j > S(i), the start of the sequence that holds i."""
    n = len(q)
    qe = [int(q[i]) + int(L[i]) for i in range(n)]
    re = [int(r[i]) + int(L[i]) for i in range(n)]
    f, pred, gain = [0] * n, [C.NONE] * n, [0] * n
    for i in range(n):
        S_i = start[seq_of(start, int(r[i]))]
        best, p, g = P.match_w * int(L[i]), C.NONE, int(L[i])
        for j in range(i - 1, max(0, i - P.lookback) - 1, -1):
            vg = C.link(P, qe[i], re[i], int(L[i]), qe[j], re[j], f[j]) if re[j] > S_i else None
            if vg is not None and vg[0] > best:
                best, p, g = vg[0], j, vg[1]
        f[i], pred[i], gain[i] = best, p, g
    return f, pred, gain


def chain_bounded(P: C.Params, q, r, L, start):
    """One problem -> dict(f, pred, gain, chains): the bounded fill, then chaining_ref's picking and output."""
    f, pred, gain = fill_bounded(P, q, r, L, start)
    return dict(f=f, pred=pred, gain=gain, chains=C.pick(P, q, r, L, f, pred, gain))


def exhaustive_best_bounded(P: C.Params, q, r, L, start):
    """The best score over every admissible subsequence of the anchors of one sequence, over the sequences (small n only)."""
    best = None
    for s in range(len(start) - 1):
        idx = [i for i in range(len(q)) if start[s + 1] > start[s] and start[s] <= int(r[i]) < start[s + 1]]
        if idx:
            b = C.exhaustive_best(P, [q[i] for i in idx], [r[i] for i in idx], [L[i] for i in idx])
            best = b if best is None or b > best else best
    return best


def chain_windows_seqs(q_len, anchor_first, q_anchor, r_anchor, anchor_len, margin: int, seq_off, seq_len):
    """-> (r_off, r_len, r_anchor, seq, shift) as ba_chain_windows_seqs writes them, in Python's integers."""
    start = [0] + np.cumsum(np.asarray(seq_len, np.int64)).tolist()
    r_off_w, r_len_w, r_anchor_w, seq, shift = [], [], [int(x) for x in r_anchor], [], []
    for c in range(len(q_len)):
        a0, a1 = int(anchor_first[c]), int(anchor_first[c + 1])
        if a1 <= a0:
            raise ValueError(f"chain {c} has no anchors")
        s = seq_of(start, int(r_anchor[a0]))
        S_, E = start[s], start[s + 1]
        for a in range(a0, a1):
            if int(q_anchor[a]) + int(anchor_len[a]) > int(q_len[c]) or int(r_anchor[a]) + int(anchor_len[a]) > E:
                raise ValueError(f"chain {c}: anchor {a - a0} ends outside its sequences")
        qa0, ra0 = int(q_anchor[a0]), int(r_anchor[a0])
        qe, re = int(q_anchor[a1 - 1]) + int(anchor_len[a1 - 1]), int(r_anchor[a1 - 1]) + int(anchor_len[a1 - 1])
        lo = ra0 - min(ra0 - S_, qa0 + margin)
        hi = re + min(E - re, (int(q_len[c]) - qe) + margin)
        r_off_w.append(int(seq_off[s]) + (lo - S_))
        r_len_w.append(hi - lo)
        seq.append(s)
        shift.append(lo - S_)
        for a in range(a0, a1):
            r_anchor_w[a] -= lo
    return (np.array(r_off_w, np.uint64), np.array(r_len_w, np.uint32), np.array(r_anchor_w, np.uint32), np.array(seq, np.uint32),
            np.array(shift, np.uint32))


def locate(seq_len, r_start, r_end):
    """-> dict(seq, local_start, local_end, crosses) as ba_ref_locate writes them, in Python's integers."""
    start = [0] + np.cumsum(np.asarray(seq_len, np.int64)).tolist()
    out = dict(seq=[], local_start=[], local_end=[], crosses=[])
    for i, (a, b) in enumerate(zip(r_start, r_end)):
        a, b = int(a), int(b)
        if b < a or b > start[-1]:
            raise ValueError(f"interval {i}")
        s = seq_of(start, a)
        out["seq"].append(s); out["local_start"].append(a - start[s]); out["local_end"].append(b - start[s]); out["crosses"].append(int(b > start[s + 1]))
    return {k: np.array(v, np.uint8 if k == "crosses" else np.uint32) for k, v in out.items()}


# ------------------------------------------------------------------ sequence sets around the seams of the sketch
def seam_sets(k: int, w: int):
    """-> {name: [bytes]}: pairs and triples of index_ref.seam_references, so that a junction falls at SPAN - 1, SPAN and SPAN + 1 windows
    of the sequence before it, with the short ones (empty, shorter than k, exactly k, one window) between long ones; poly-A on both sides
    of a junction (the junction would form valid k-mers and a minimizer if the bound leaked); and 2000 sequences of 0 .. 40 bytes."""
    R = X.seam_references(k, w)
    rng = np.random.default_rng(71 + 100 * k + w)
    out = {}
    for nw in (X.SPAN - 1, X.SPAN, X.SPAN + 1):
        out[f"pair_{nw}"] = [R[f"random_{nw}"], R["random_%d" % (2 * X.SPAN + 1)]]
    out["triple_short_between"] = [R["random_%d" % X.SPAN], R["empty"], R["random_%d" % (X.SPAN + 1)], R["shorter_than_k"], R["random_%d" % (X.SPAN - 1)]]
    out["triple_one_k_mer_between"] = [R["random_%d" % (X.SPAN + 1)], R["exactly_k"], R["random_%d" % X.SPAN], R["one_window"], R["n_run"],
                                       R["fewer_k_mers_than_w"]]
    out["short_ones_first_and_last"] = [R["empty"], R["exactly_k"], R["random_%d" % X.SPAN], R["all_t"], R["empty"]]
    a = S.dna(rng, X.ref_len_for_windows(X.SPAN, k, w) - 100) + b"A" * 100
    out["poly_a_across_the_junction"] = [a, b"A" * 100 + S.dna(rng, 700)]
    out["many_short"] = [S.dna(rng, int(n)) for n in rng.integers(0, 41, 2000)]
    return out


def cap_sum_case(k: int, max_occ: int, max_ref_occ: int, seed: int = 73):
    """With w = 1, in the manner of index_ref.occ_case: one k-mer that the first sequence holds max_ref_occ times and the third once -- only
    the sum is over the cap --, and one that they hold once and max_ref_occ - 1 times: exactly at it. The read holds each max_occ times
    -> (sequences: the two, an empty one between them and a short one behind; ReadSet)."""
    rng = np.random.default_rng(seed)
    gap = lambda: S.dna(rng, 31)   # noqa: E731
    over, at = S.dna(rng, k), S.dna(rng, k)
    put = lambda mer, n: b"".join(b"N" + mer + b"N" + gap() for _ in range(n))   # noqa: E731
    a = gap() + put(over, max_ref_occ) + put(at, 1)
    b = gap() + put(over, 1) + put(at, max_ref_occ - 1)
    read = gap() + put(over, max_occ) + put(at, max_occ)
    return [a, b"", b, S.dna(rng, k - 1)], X.ReadSet([(read, 0), (S.oriented(read, 1), 1), (read[:len(read) // 2], 0)])


# ------------------------------------------------------------------ chaining across a junction
JUNCTION_PARAMS = C.Params(4, 1, 0, 64, 400, 60, 4, 24, 1)
JUNCTION_START = [0, 1000, 1000, 3000]   # three sequences, the middle one empty: the junction is at 1000


def junction_problem():
    """Anchors of 12 bases every 20 on one diagonal, from 880 to 1100 on the reference: colinear across the junction at 1000, well inside
    max_dist and bandwidth, and none straddles it (960 .. 972, then 1000 .. 1012) -> (q, r, L)."""
    r = [x for x in range(880, 1101, 20) if not (x < 1000 < x + 12)]
    return [x - 800 for x in r], r, [12] * len(r)


def drop_straddlers(q, r, L, start):
    """The anchors that lie inside one sequence."""
    keep = [i for i in range(len(q)) if seq_of(start, int(r[i])) == seq_of(start, int(r[i]) + int(L[i]) - 1)]
    return [q[i] for i in keep], [r[i] for i in keep], [L[i] for i in keep]


def diagonal_problem(n: int, step: int = 5, L: int = 4):
    """n anchors along one diagonal, every `step` bases and shorter than that, so that none straddles a junction put where one starts:
    each one's best predecessor is the one before it."""
    return [10 + step * i for i in range(n)], [30 + step * i for i in range(n)], [L] * n


def bounded_sets():
    """The problem sets of the bounded fill, by name -> (Params, ProblemSet, start): the junction problem; chaining_ref.gpu_sets()-style
    random problems split at random junctions; a problem longer than 64 anchors with a junction inside a chunk; and one with a junction
    where the look-back ring (128 slots for a look-back of 64) wraps. One table per set: every problem of a set lies in its frame."""
    rng = np.random.default_rng(2025)
    P = C.Params(4, 1, 1, 64, 400, 60, 4, 24, 2)
    out = dict(junction=(JUNCTION_PARAMS, C.ProblemSet([junction_problem()]), JUNCTION_START))
    probs, cuts = [], set()
    for n in (0, 1, 63, 64, 65, 2, 130, 300):
        q, r, L = C.random_problem(rng, n)
        probs.append((q, r, L))
        if n > 1:
            cuts |= set(int(x) for x in rng.integers(1, max(r) + 1, 3))
    cuts = sorted(cuts)
    start = [0] + cuts + [cuts[-1], 1 << 20]   # (an empty sequence before the last)
    probs = [drop_straddlers(q, r, L, start) for q, r, L in probs]
    out["random"] = (P, C.ProblemSet(probs), start)
    # anchor i of diagonal_problem covers the reference from 30 + 5 i: a junction at 30 + 5 * 100 lies before anchor 100, inside the second
    # chunk of 64; one at 30 + 5 * 128 before anchor 128, the first anchor whose ring slot is slot 0 again
    q, r, L = diagonal_problem(200)
    out["inside_a_chunk"] = (P, C.ProblemSet([(q, r, L), diagonal_problem(70)]), [0, 30 + 5 * 100, 1 << 20])
    out["at_the_ring_wrap"] = (P, C.ProblemSet([(q, r, L)]), [0, 30 + 5 * 128, 30 + 5 * 130, 1 << 20])
    return out


# ------------------------------------------------------------------ the whole path: reads drawn from several sequences
MAP_LENGTHS = (4000, 300, 0, 6000)
MAP_NAMES = ("chr_a", "contig_b", "nothing", "chr_d")
READ_LEN = 600


class MultiMappingSet:
    """Sequences of 4000, 300, 0 and 6000 bases and twelve reads of about 600 with 5 % edits, every read listed on both strands (problem
    2 i is read i on strand 0, problem 2 i + 1 on strand 1). Read 0 comes from the last 600 bases of the first sequence, read 1 from the first
    600 of the last one; the last read is chimeric: its first half is the end of the 300-base sequence, its second half the start of the
    6000-base one, which are adjacent in the index's frame because the empty sequence sits between them. origin[i] = (seq, start, end,
    strand) in the sequence's own coordinates; the chimeric read has none."""

    def __init__(self, seed: int = 59):
        rng = np.random.default_rng(seed)
        self.seqs = [S.dna(rng, n) for n in MAP_LENGTHS]
        self.start = seq_start(self.seqs)
        places = [(0, MAP_LENGTHS[0] - READ_LEN), (3, 0)]
        while len(places) < 11:
            s = 0 if len(places) % 2 else 3
            places.append((s, int(rng.integers(0, MAP_LENGTHS[s] - READ_LEN))))
        reads, self.origin = [], []
        for i, (s, a) in enumerate(places):
            read = S.oriented(S.mutate(rng, self.seqs[s][a:a + READ_LEN], 0.05), i % 2)
            reads += [(read, 0), (read, 1)]
            self.origin.append((s, a, a + READ_LEN, i % 2))
        chim = S.mutate(rng, self.seqs[1][-280:] + self.seqs[3][:320], 0.05)
        reads += [(chim, 0), (chim, 1)]
        self.chimeric = len(places)
        self.reads = X.ReadSet(reads)
        # the caller's pool: the reads, then the sequences in another order and apart from one another
        order = (3, 0, 2, 1)
        off, pool = {}, self.reads.pool.tobytes()
        for s in order:
            pool += b"#" * 5
            off[s] = len(pool)
            pool += self.seqs[s]
        self.pool = np.frombuffer(pool + b"#" * 8, np.uint8).copy()
        self.seq_off = np.array([off[s] for s in range(len(self.seqs))], np.uint64)
        self.seq_len = np.array(MAP_LENGTHS, np.uint32)

    def true_problem(self, i: int) -> int:
        return 2 * i + self.origin[i][3]

    def expected_hits(self):
        return [hits_multi(q, self.seqs, X.MAP_PARAMS, s) for q, s in self.reads.reads]


def model_chains(exps, start, CP=X.MAP_CHAINING, k=X.MAP_PARAMS.k):
    """The bounded chaining model over the model's hits -> the chains as ba_chaining_results orders them: [(problem, rank, [(qa, ra, len)])]."""
    cps = C.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), k)) for e in exps])
    out = []
    for p, (q, r, L) in enumerate(cps.problems):
        for rank, (_, anchors) in enumerate(chain_bounded(CP, q, r, L, start)["chains"]):
            out.append((p, rank, [(qa, ra, g) for qa, ra, g, _ in anchors]))
    return out


def windowed_chain_set(ms: MultiMappingSet, chains, margin: int = X.MAP_MARGIN):
    """The chains cut to their candidate windows by the model, as a tests/chain_ref.py chain set whose references are the windows' bytes
    -> (ChainSet, seq, shift)."""
    from tests import chain_ref
    rs = ms.reads
    q_len = [int(rs.q_len[p]) for p, _, _ in chains]
    first = np.concatenate([[0], np.cumsum([len(a) for _, _, a in chains])])
    flat = [x for _, _, a in chains for x in a]
    r_off, r_len, r_anchor, seq, shift = chain_windows_seqs(q_len, first, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat], margin,
                                                            ms.seq_off, ms.seq_len)
    seqs = [q for q, _ in rs.reads] + [ms.pool[int(o):int(o) + int(n)].tobytes() for o, n in zip(r_off, r_len)]
    found = []
    for c, (p, _, anchors) in enumerate(chains):
        a0 = int(first[c])
        found.append((p, len(rs) + c, [(qa, int(r_anchor[a0 + i]), g) for i, (qa, _, g) in enumerate(anchors)], rs.reads[p][1]))
    return chain_ref.ChainSet(seqs, found, True), seq, shift
