#!/usr/bin/env python3
"""Anchor-chain rate on the GPU: 10 kbp DNA reads against their reference stretch, an exact 15-base anchor every few hundred bases (at true shared
positions; the stretches between them differ by ~10 % edits), global alignment between the anchors, X-drop at both ends.
  chain batch:       ChainBatchAligner -- every piece cut on the device, the ends' fill, the gaps' fill, the segmented splice on the device
  host composition:  the same work from the calls that existed before: the gap slices cut in NumPy into a pool of their own, one global
                     BatchAligner over them, one ExtendBatchAligner over the end anchors (two seeds per chain: the first anchor on the
                     sequences cut behind it, the last anchor on the sequences cut before it), the anchors scored and everything spliced in NumPy
Prints the device times (packers, both fills, splice), end to end (create -> cigars) for both, and checks that the two agree; writes the
same to profiles/chain_rate.json.
usage: chain_rate.py [chains] [runs]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from block_aligner_amd import hip as H, scores as S, synth   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
runs_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
size, x_drop, mode, gaps, L = (32, 256), 100, H.TRACE | H.X_DROP, (-5, -1), 15
m = S.NucMatrix.new_simple(2, -3)
rng = np.random.default_rng(1234)

# ---- the workload: per chain a read and a reference of ~10 kbp, anchors of L bases at shared positions
seqs, first, qa, ra = [], [0], [], []
for c in range(n):
    read, ref, qn, rn = [], [], 0, 0
    for k in range(int(rng.integers(28, 40))):
        g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)   # the stretch before anchor k (before the first one: the left end)
        h = synth.mutate(rng, g, len(g) // 10, synth.DNA)
        a = synth.rand_str(rng, L, synth.DNA)
        qa.append(qn + len(h)); ra.append(rn + len(g))
        read += [h, a]; ref += [g, a]
        qn += len(h) + L; rn += len(g) + L
    g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
    read.append(synth.mutate(rng, g, len(g) // 10, synth.DNA)); ref.append(g)
    seqs += [np.concatenate(read), np.concatenate(ref)]
    first.append(len(qa))
lens = np.array([len(s) for s in seqs], np.int64)
offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
pool = np.concatenate(seqs + [np.zeros(8, np.uint8)])
q_off, q_len, r_off, r_len = offs[0::2], lens[0::2], offs[1::2], lens[1::2]
first = np.array(first, np.int64)
qa, ra = np.array(qa, np.int64), np.array(ra, np.int64)
al = np.full(len(qa), L, np.int64)
K = np.diff(first)
assert (K >= 2).all()   # (the host composition below takes the two ends from two different anchors)
out = dict(chains=n, anchors=int(len(qa)), bases=int(lens.sum()), size=size, x_drop=x_drop, mode="TRACE|X_DROP", anchor_len=L)

# ---- the chain batch
def chain_batch():
    t0 = time.perf_counter()
    cb = H.ChainBatchAligner(m, gaps, size, x_drop, mode, pool, q_off, q_len, r_off, r_len, first, qa, ra, al)
    cb.run()
    res = cb.results()
    runs, off = cb.cigars(res["cigar_len"])
    e2e = (time.perf_counter() - t0) * 1e3
    pack_ms = cb.times()["pack_ms"]
    tt = []
    for _ in range(runs_timed):
        cb.run(); tt.append(cb.times())
    assert not res["status"].any()
    med = lambda k: float(np.median([t[k] for t in tt]))   # noqa: E731
    cb.close()
    return dict(pack_ms=pack_ms, ends_ms=med("ends_ms"), gaps_ms=med("gaps_ms"), splice_ms=med("splice_ms"), end_to_end_ms=e2e,
                cells=int(res["cells"].sum())), res, runs


# ---- the host composition
def host_composition():
    t0 = time.perf_counter()
    chain_of = np.repeat(np.arange(n), K)
    inner = np.ones(len(qa), bool); inner[first[1:] - 1] = False          # anchors with a gap behind them
    g_q0, g_r0 = (qa + al)[inner], (ra + al)[inner]
    g_ql, g_rl = qa[1:][inner[:-1]] - g_q0, ra[1:][inner[:-1]] - g_r0
    g_chain = chain_of[inner]
    assert (g_ql > 0).all() and (g_rl > 0).all()                         # (this workload: every gap has bytes on both sides)
    # the gap slices into a pool of their own, as a caller without device-side cutting has to
    take = lambda o, ln: np.repeat(o, ln) + (np.arange(ln.sum()) - np.repeat(np.cumsum(ln) - ln, ln))   # noqa: E731
    gq_bytes, gr_bytes = pool[take(q_off[g_chain] + g_q0, g_ql)], pool[take(r_off[g_chain] + g_r0, g_rl)]
    gap_pool = np.concatenate([gq_bytes, gr_bytes, np.zeros(8, np.uint8)])
    gq_off, gr_off = np.cumsum(g_ql) - g_ql, len(gq_bytes) + np.cumsum(g_rl) - g_rl
    t_cut = (time.perf_counter() - t0) * 1e3
    gb = H.BatchAligner(m, gaps, size, 0, H.TRACE, gap_pool, gq_off, g_ql, gr_off, g_rl)
    gaps_host_ms = gb.run()
    gres = gb.results()
    gruns, goff = gb.cigars(gres["cigar_len"])
    # the ends: seed 2c = the first anchor on the sequences cut behind it, seed 2c + 1 = the last anchor on the sequences cut before it
    fa, la = first[:-1], first[1:] - 1
    e_qo = np.stack([q_off, q_off + qa[la]], 1).ravel(); e_ql = np.stack([qa[fa] + L, q_len - qa[la]], 1).ravel()
    e_ro = np.stack([r_off, r_off + ra[la]], 1).ravel(); e_rl = np.stack([ra[fa] + L, r_len - ra[la]], 1).ravel()
    e_qs = np.stack([qa[fa], np.zeros(n, np.int64)], 1).ravel(); e_rs = np.stack([ra[fa], np.zeros(n, np.int64)], 1).ravel()
    eb = H.ExtendBatchAligner(m, gaps, size, x_drop, mode, pool, e_qo, e_ql, e_ro, e_rl, e_qs, e_rs, np.full(2 * n, L))
    ends_host_ms = eb.run()
    eres = eb.results()
    eruns, eoff = eb.cigars(eres["cigar_len"])
    t1 = time.perf_counter()
    # splice: per chain the left seed's runs (they end with the first anchor's M), the gaps and the later anchors in turn, the right seed's runs
    # (they start with the last anchor's M)
    a_score = 2 * L
    score = eres["score"][0::2].astype(np.int64) + eres["score"][1::2] + np.bincount(g_chain, gres["score"], n).astype(np.int64) + (K - 2) * a_score
    mid = np.full(len(qa), (L << 4) | 1, np.uint32)                      # every anchor as one M run
    src = np.concatenate([eruns, gruns, mid])
    GB, MB = len(eruns), len(eruns) + len(gruns)
    # elements per chain, 2 K - 1 of them: the left seed, then gap 0, anchor 1, gap 1, ..., gap K - 2, the right seed
    ne = 2 * K - 1
    el_chain = np.repeat(np.arange(n), ne)
    pos = np.arange(ne.sum()) - np.repeat(np.cumsum(ne) - ne, ne)
    is_l, is_r, is_gap = pos == 0, pos == ne[el_chain] - 1, (pos & 1) == 1
    anchor = first[el_chain] + pos // 2                                  # the gap's anchor (odd positions) / the anchor itself (even ones)
    gi = (np.cumsum(inner) - 1)[np.minimum(anchor, len(qa) - 1)]         # anchor -> its gap's index
    eoff, goff = eoff.astype(np.int64), goff.astype(np.int64)
    starts = np.where(is_l, eoff[2 * el_chain], np.where(is_r, eoff[2 * el_chain + 1], np.where(is_gap, GB + goff[gi], MB + anchor)))
    counts = np.where(is_l, eoff[2 * el_chain + 1] - eoff[2 * el_chain], np.where(is_r, eoff[2 * el_chain + 2] - eoff[2 * el_chain + 1],
                                                                                    np.where(is_gap, goff[gi + 1] - goff[gi], 1)))
    cat = src[take(starts, counts)]
    owner = np.repeat(el_chain, counts)
    new = np.ones(len(cat), bool)
    new[1:] = ((cat[1:] & 15) != (cat[:-1] & 15)) | (owner[1:] != owner[:-1])
    grp = np.flatnonzero(new)
    hruns = (np.add.reduceat((cat >> 4).astype(np.uint64), grp).astype(np.uint32) << 4) | (cat[grp] & 15)
    hcnt = np.bincount(owner[grp], minlength=n)
    t_splice = (time.perf_counter() - t1) * 1e3
    e2e_host = (time.perf_counter() - t0) * 1e3
    hcells = int(gres["cells"].sum() + eres["cells"].sum())
    gb.close(); eb.close()
    return dict(host_cut_ms=t_cut, ends_ms=ends_host_ms, gaps_ms=gaps_host_ms, numpy_splice_ms=t_splice, end_to_end_ms=e2e_host, cells=hcells), score, hcnt, hruns


# ---- one untimed pass of both (the first use of the device: context, code objects, the allocator's first blocks), then both `runs` times in
# turn; end to end is the median
chain_batch(); host_composition()
dev, hst = [], []
for _ in range(runs_timed):
    dev.append(chain_batch()); hst.append(host_composition())
pick = lambda xs: sorted(xs, key=lambda x: x[0]["end_to_end_ms"])[len(xs) // 2]   # noqa: E731
(c, res, runs), (h, score, hcnt, hruns) = pick(dev), pick(hst)
out["chain_batch"], out["host_composition"] = c, h
out["end_to_end_ms_all"] = dict(chain_batch=[d[0]["end_to_end_ms"] for d in dev], host_composition=[x[0]["end_to_end_ms"] for x in hst])
cells, hcells, e2e, e2e_host = c["cells"], h["cells"], c["end_to_end_ms"], h["end_to_end_ms"]
out["agree"] = bool(np.array_equal(score, res["score"]) and np.array_equal(hcnt, res["cigar_len"]) and np.array_equal(hruns, runs) and hcells == cells)
out["splice_and_pack_over_fills"] = (c["pack_ms"] + c["splice_ms"]) / max(c["ends_ms"] + c["gaps_ms"], 1e-9)
out["host_over_device_end_to_end"] = e2e_host / e2e
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "chain_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
