#!/usr/bin/env python3
"""Per-alignment statistics rate on the GPU: config 3 (10 kbp DNA reads, block 128..1024, X-drop 100), TRACE|X_DROP with and
without CIGAR_EQ.
  device: BatchAligner.stats() -- k_stats over the runs and images the fill left on the device (its HIP-event time beside the fill's)
  NumPy:  the same records computed on the host from cigars() and the raw sequences, as a caller does without the feature
Prints kernel, fill and NumPy times and checks that the two agree field by field.
usage: stats_rate.py [pairs] [runs]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from block_aligner_amd import hip as H, verify, workloads as W   # noqa: E402

FIELDS = ("q_start", "r_start", "columns", "matches", "mismatches", "positives", "ins", "del", "gap_opens", "longest_ins", "longest_del", "path_score")


def numpy_stats(pairs, matrix, gaps, res, runs, off, chunk=1000):
    """The ba_batch_stats records of a traced batch, in NumPy: every match-type column expanded and both bytes compared, a chunk of pairs at a time."""
    n = len(pairs)
    tab = verify.score_table(matrix)
    up = np.arange(256)
    if getattr(matrix, "KIND", 1) != 2:
        up = verify._upper(up)
    out = {k: np.zeros(n, np.int64) for k in FIELDS}
    pool = pairs.pool
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        x = runs[int(off[a]):int(off[b])].astype(np.int64)
        cnt = np.diff(off[a:b + 1].astype(np.int64))
        owner = np.repeat(np.arange(a, b), cnt)
        ops, lens = x & 15, x >> 4
        m, gi, gd = ops <= 3, ops == 4, ops == 5
        cq, cr = np.where(m | gi, lens, 0), np.where(m | gd, lens, 0)
        qs = res["query_idx"][a:b].astype(np.int64) - np.bincount(owner - a, cq, minlength=b - a).astype(np.int64)
        rs = res["reference_idx"][a:b].astype(np.int64) - np.bincount(owner - a, cr, minlength=b - a).astype(np.int64)
        first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        eq_, er_ = np.cumsum(cq) - cq, np.cumsum(cr) - cr   # consumed before each run, over the chunk
        i0 = qs[owner - a] + eq_ - np.repeat(eq_[first[cnt > 0]], cnt[cnt > 0])
        j0 = rs[owner - a] + er_ - np.repeat(er_[first[cnt > 0]], cnt[cnt > 0])
        ml = lens[m]
        cell_owner = np.repeat(owner[m], ml)
        within = np.arange(int(ml.sum())) - np.repeat(np.cumsum(ml) - ml, ml)
        qa = up[pool[pairs.q_off[cell_owner].astype(np.int64) + np.repeat(i0[m], ml) + within]]
        ra = up[pool[pairs.r_off[cell_owner].astype(np.int64) + np.repeat(j0[m], ml) + within]]
        s = tab[qa, ra]
        k = cell_owner - a
        sl = slice(a, b)
        out["q_start"][sl], out["r_start"][sl] = qs, rs
        out["columns"][sl] = np.bincount(owner - a, lens, minlength=b - a)
        out["matches"][sl] = np.bincount(k, qa == ra, minlength=b - a)
        out["mismatches"][sl] = np.bincount(k, qa != ra, minlength=b - a)
        out["positives"][sl] = np.bincount(k, s > 0, minlength=b - a)
        out["ins"][sl] = np.bincount(owner - a, np.where(gi, lens, 0), minlength=b - a)
        out["del"][sl] = np.bincount(owner - a, np.where(gd, lens, 0), minlength=b - a)
        out["gap_opens"][sl] = np.bincount(owner - a, gi | gd, minlength=b - a)
        np.maximum.at(out["longest_ins"], owner[gi], lens[gi])
        np.maximum.at(out["longest_del"], owner[gd], lens[gd])
        gap = np.where(gi | gd, gaps[0] + gaps[1] * (lens - 1), 0)
        out["path_score"][sl] = np.bincount(k, s, minlength=b - a) + np.bincount(owner - a, gap, minlength=b - a)
    return out


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    runs_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    w = W.config3(n, workers=16)
    p = w.pairs
    size, x_drop = (128, 1024), w.x_drop
    out = dict(pairs=n, size=size, x_drop=x_drop)
    host = {}
    for name, mode in (("TRACE|X_DROP", H.TRACE | H.X_DROP), ("TRACE|X_DROP|CIGAR_EQ", H.TRACE | H.X_DROP | H.CIGAR_EQ)):
        b = H.BatchAligner(w.matrix, w.gaps, size, x_drop, mode, p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
        fill = b.run()
        res = b.results()
        assert not res["status"].any()
        st = b.stats()
        kms = []
        for _ in range(runs_timed):
            b.stats()
            kms.append(b.stats_ms())
        t0 = time.perf_counter()
        runs, off = b.cigars(res["cigar_len"])
        t_cig = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        ref = numpy_stats(p, w.matrix, w.gaps, res, runs, off)
        t_np = (time.perf_counter() - t0) * 1e3
        agree = all(np.array_equal(st[k].astype(np.int64), ref[k]) for k in FIELDS) and np.array_equal(st["path_score"], res["score"])
        host[name] = st
        out[name] = dict(fill_ms=fill, stats_kernel_ms=float(np.median(kms)), stats_kernel_ms_min=float(np.min(kms)), stats_kernel_pct_of_fill=100.0 * float(np.median(kms)) / fill,
                         cigars_copy_ms=t_cig, numpy_stats_ms=t_np, columns=int(st["columns"].sum()), match_columns=int((st["matches"] + st["mismatches"]).sum()),
                         mean_identity=float(st["identity"].mean()), agree=bool(agree))
        b.close()
    a, c = host.values()
    out["modes_agree"] = all(np.array_equal(a[k], c[k]) for k in FIELDS)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
