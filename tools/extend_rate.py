#!/usr/bin/env python3
"""Seed-and-extend rate on the GPU: one seed in the middle of every pair of config 3 (10 kbp DNA reads), X-drop both ways.
  extension batch: ExtendBatchAligner -- the sides' images cut on the device, one fill, the splice on the device
  host-side path:  reversed prefixes built on the host, a plain BatchAligner over the same 2N sides, the seeds scored and the CIGARs spliced
                   in NumPy
Prints fill kernel time, packer / splice time, end to end (create -> cigars) and GCUPS on the cells of both, and checks that the two agree.
usage: extend_rate.py [seeds] [runs]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from block_aligner_amd import hip as H, scores as S, workloads as W   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
runs_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
w = W.config3(n, workers=16)
p = w.pairs
size, x_drop, mode, gaps, L = (128, 1024), 100, H.TRACE | H.X_DROP | H.CIGAR_EQ, w.gaps, 20
m = w.matrix
q_len, r_len = p.q_len.astype(np.int64), p.r_len.astype(np.int64)
q_seed = np.minimum(q_len // 2, q_len - L).astype(np.uint32)
r_seed = np.minimum(r_len // 2, r_len - L).astype(np.uint32)
seed_len = np.full(n, L, np.uint32)
out = dict(seeds=n, size=size, x_drop=x_drop, mode="TRACE|X_DROP|CIGAR_EQ")


def gcups(cells, ms):
    return cells / (ms * 1e-3) / 1e9


# ---- the extension batch
t0 = time.perf_counter()
eb = H.ExtendBatchAligner(m, gaps, size, x_drop, mode, p.pool, p.q_off, p.q_len, p.r_off, p.r_len, q_seed, r_seed, seed_len)
eb.run()
res = eb.results()
runs, off = eb.cigars(res["cigar_len"])
e2e = (time.perf_counter() - t0) * 1e3
t = eb.times()
fills, splices = [], []
for _ in range(runs_timed):
    fills.append(eb.run()); splices.append(eb.times()["splice_ms"])
cells = int(res["cells"].sum())
assert not res["status"].any()
out["extension"] = dict(fill_ms=float(np.median(fills)), pack_ms=t["pack_ms"], splice_ms=float(np.median(splices)), end_to_end_ms=e2e,
                        cells=cells, gcups_fill=gcups(cells, np.median(fills)), gcups_end_to_end=gcups(cells, e2e))
eb.close()

# ---- the host-side path: reversed prefixes on the host, a plain batch over the 2N sides, splice in NumPy
t0 = time.perf_counter()
pool = p.pool
qo, ro = p.q_off.astype(np.int64), p.r_off.astype(np.int64)
ql_l, rl_l = q_seed.astype(np.int64), r_seed.astype(np.int64)
ql_r, rl_r = q_len - q_seed - L, r_len - r_seed - L
has_l = (ql_l > 0) & (rl_l > 0)
has_r = (ql_r > 0) & (rl_r > 0)
# side pool: every left query / reference prefix reversed, the right sides as they are
pieces, sq_off, sq_len, sr_off, sr_len, side_of = [], [], [], [], [], []
at = 0
for s in range(n):
    for w_, ok in ((0, has_l[s]), (1, has_r[s])):
        if not ok:
            continue
        if w_ == 0:
            a, b = pool[qo[s]:qo[s] + ql_l[s]][::-1], pool[ro[s]:ro[s] + rl_l[s]][::-1]
        else:
            a = pool[qo[s] + q_seed[s] + L:qo[s] + q_len[s]]
            b = pool[ro[s] + r_seed[s] + L:ro[s] + r_len[s]]
        pieces += [a, b]
        sq_off.append(at); sq_len.append(len(a)); at += len(a)
        sr_off.append(at); sr_len.append(len(b)); at += len(b)
        side_of.append(2 * s + w_)
side_pool = np.concatenate(pieces)
t_rev = (time.perf_counter() - t0) * 1e3
b = H.BatchAligner(m, gaps, size, x_drop, mode, side_pool, sq_off, sq_len, sr_off, sr_len)
fill_host = b.run()
sres = b.results()
sruns, soff = b.cigars(sres["cigar_len"])
t1 = time.perf_counter()
# seeds: scores and =/X runs
qs_b = pool[(qo + q_seed)[:, None] + np.arange(L)]
rs_b = pool[(ro + r_seed)[:, None] + np.arange(L)]
seed_score = m.raw()[(qs_b.astype(np.int64) & 7) * 16 + (rs_b.astype(np.int64) & 15)].astype(np.int64).sum(1)
sop = np.where(qs_b == rs_b, 2, 3).astype(np.uint32).ravel()
start = np.ones(n * L, bool)
start[1:] = sop[1:] != sop[:-1]
start[::L] = True
rid = np.cumsum(start) - 1
seed_runs = (np.bincount(rid).astype(np.uint32) << 4) | sop[start]
seed_cnt = np.add.reduceat(start.astype(np.int64), np.arange(0, n * L, L))
# per side -> per seed
side_idx = np.full(2 * n, -1, np.int64)
side_idx[np.array(side_of)] = np.arange(len(side_of))
score = seed_score.copy()
cnt = np.zeros((n, 2), np.int64)
for w_ in (0, 1):
    i = side_idx[w_::2]
    ok = i >= 0
    score[ok] += sres["score"][i[ok]]
    cnt[ok, w_] = sres["cigar_len"][i[ok]]
# the spliced runs: left runs reversed, seed runs, right runs; then equal neighbours within a seed merged
src = np.concatenate([sruns, seed_runs])
seed_off = np.concatenate([[0], np.cumsum(seed_cnt)[:-1]]) + len(sruns)
lo_ = np.where(side_idx[0::2] >= 0, soff[:-1][np.maximum(side_idx[0::2], 0)].astype(np.int64), 0)
ro_ = np.where(side_idx[1::2] >= 0, soff[:-1][np.maximum(side_idx[1::2], 0)].astype(np.int64), 0)
tot = cnt[:, 0] + seed_cnt + cnt[:, 1]
owner = np.repeat(np.arange(n), tot)
k = np.arange(tot.sum()) - np.repeat(np.concatenate([[0], np.cumsum(tot)[:-1]]), tot)
nl, ns = cnt[owner, 0], seed_cnt[owner]
idx = np.where(k < nl, lo_[owner] + nl - 1 - k, np.where(k < nl + ns, seed_off[owner] + k - nl, ro_[owner] + k - nl - ns))
cat = src[idx]
new = np.ones(len(cat), bool)
new[1:] = ((cat[1:] & 15) != (cat[:-1] & 15)) | (owner[1:] != owner[:-1])
grp = np.flatnonzero(new)
hruns = (np.add.reduceat((cat >> 4).astype(np.uint64), grp).astype(np.uint32) << 4) | (cat[grp] & 15)
hcnt = np.bincount(owner[grp], minlength=n)
t_splice = (time.perf_counter() - t1) * 1e3
e2e_host = (time.perf_counter() - t0) * 1e3
hcells = int(sres["cells"].sum())
out["host_path"] = dict(fill_ms=fill_host, host_reverse_ms=t_rev, numpy_splice_ms=t_splice, end_to_end_ms=e2e_host, cells=hcells,
                        gcups_fill=gcups(hcells, fill_host), gcups_end_to_end=gcups(hcells, e2e_host))
b.close()
out["agree"] = bool(np.array_equal(score, res["score"]) and np.array_equal(hcnt, res["cigar_len"]) and np.array_equal(hruns, runs) and hcells == cells)
print(json.dumps(out))
