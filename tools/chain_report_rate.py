#!/usr/bin/env python3
"""What describing the alignments of a chain batch costs, on the workload of tools/chain_rate.py: 2000 chains of 10 kbp DNA reads, an exact
15-base anchor every few hundred bases, ~10 % edits between them, 32..256, TRACE | X_DROP | CIGAR_EQ. After the batch has run:
  device path:  report().stats() and report().text() for CIGAR, MD and cs -- k_stats over the pieces, k_stats_chain, the text kernels, and
                the copies of records and text to the host
  host path:    the same four products as a caller had to make them before: results() and cigars() downloaded, the statistics in vectorised
                NumPy over the = / X / I / D runs, the three strings per chain in Python from the runs and the sequences
Both paths in this process and run, after one untimed pass of both; medians of three. The products must be equal. Prints one JSON line and
writes profiles/chain_report_rate.json.
usage: chain_report_rate.py [chains] [runs]"""
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
size, x_drop, mode, gaps, L = (32, 256), 100, H.TRACE | H.X_DROP | H.CIGAR_EQ, (-5, -1), 15
MATCH, MISMATCH = 2, -3
m = S.NucMatrix.new_simple(MATCH, MISMATCH)
rng = np.random.default_rng(1234)

# ---- the workload of tools/chain_rate.py: per chain a read and a reference of ~10 kbp, anchors of L bases at shared positions
seqs, first, qa, ra = [], [0], [], []
for c in range(n):
    read, ref, qn, rn = [], [], 0, 0
    for k in range(int(rng.integers(28, 40))):
        g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
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
out = dict(chains=n, anchors=int(len(qa)), bases=int(lens.sum()), size=size, x_drop=x_drop, mode="TRACE|X_DROP|CIGAR_EQ", anchor_len=L,
           expectation="stated before the first run: the device path (stats() and text() for CIGAR, MD and cs, copies included) at least 50 "
                       "times faster end to end than the host path (results() and cigars() downloaded, NumPy statistics, Python strings); "
                       "the report's kernels (the statistics' and the three text calls' together) under a quarter of the two fills' "
                       "device time; the statistics' kernels under a tenth of it")

cb = H.ChainBatchAligner(m, gaps, size, x_drop, mode, pool, q_off, q_len, r_off, r_len, first, qa, ra, al)
cb.run()
assert not cb.results()["status"].any()
fills_ms = cb.times()["ends_ms"] + cb.times()["gaps_ms"]
FORMATS = (("cigar", H.TEXT_CIGAR), ("md", H.TEXT_MD), ("cs", H.TEXT_CS))


# ---- the device path
def device_path():
    rep = cb.report()
    t0 = time.perf_counter()
    st = rep.stats()
    t1 = time.perf_counter()
    stats_kernel_ms = rep.ms()[0]
    texts, text_kernel_ms, text_wall = {}, {}, {}
    for name, fmt in FORMATS:
        t2 = time.perf_counter()
        off0 = np.zeros(n + 1, np.uint64)
        cb._call("text", fmt, off0.ctypes.data, None, 0)   # the two calls of text(), timed apart: sizes, then rendering
        k0 = rep.ms()[1]
        buf = np.zeros(int(off0[-1]), np.uint8)
        cb._call("text", fmt, off0.ctypes.data, buf.ctypes.data, buf.size)
        texts[name] = (buf, off0)
        text_kernel_ms[name] = k0 + rep.ms()[1]
        text_wall[name] = (time.perf_counter() - t2) * 1e3
    e2e = (time.perf_counter() - t0) * 1e3
    return dict(stats_ms=(t1 - t0) * 1e3, text_ms=text_wall, end_to_end_ms=e2e, stats_kernels_ms=stats_kernel_ms, text_kernels_ms=text_kernel_ms,
                text_bytes={k: int(v[0].size) for k, v in texts.items()}), st, texts


# ---- the host path
def host_stats(res, runs, off):
    """Vectorised over all runs of all chains: with CIGAR_EQ the = and X runs are the matches and the mismatches, and this matrix scores
    exactly the equal columns above zero."""
    off = off.astype(np.int64)
    ops, ln = (runs & 15).astype(np.int64), (runs >> 4).astype(np.int64)
    owner = np.repeat(np.arange(n), np.diff(off))
    tot = lambda mask, w=None: np.bincount(owner[mask], ln[mask] if w is None else w[mask], n).astype(np.int64)   # noqa: E731
    eq, x, i, d = ops == 2, ops == 3, ops == 4, ops == 5
    st = dict(matches=tot(eq), mismatches=tot(x), ins=tot(i), columns=tot(eq | x | i | d))
    st["del"] = tot(d)
    st["positives"] = st["matches"].copy()
    st["gap_opens"] = np.bincount(owner[i | d], minlength=n).astype(np.int64)
    for key, mask in (("longest_ins", i), ("longest_del", d)):
        v = np.zeros(n, np.int64)
        np.maximum.at(v, owner[mask], ln[mask])
        st[key] = v
    st["path_score"] = MATCH * st["matches"] + MISMATCH * st["mismatches"] + gaps[0] * st["gap_opens"] + gaps[1] * (st["ins"] + st["del"] - st["gap_opens"])
    st["q_start"] = res["q_end"].astype(np.int64) - (st["matches"] + st["mismatches"] + st["ins"])
    st["r_start"] = res["r_end"].astype(np.int64) - (st["matches"] + st["mismatches"] + st["del"])
    st["edit_distance"] = st["mismatches"] + st["ins"] + st["del"]
    st["identity"] = np.divide(st["matches"], st["columns"], out=np.zeros(n, np.float64), where=st["columns"] > 0)
    return st


def host_strings(c, runs, q_start, r_start):
    """One chain's CIGAR, MD and cs from its = / X / I / D runs and its sequences, run by run."""
    q = pool[q_off[c]:q_off[c] + q_len[c]].tobytes().decode("latin-1")
    r = pool[r_off[c]:r_off[c] + r_len[c]].tobytes().decode("latin-1")
    ql, rl = q.lower(), r.lower()
    i, j, same, cig, md, cs = q_start, r_start, 0, [], [], []
    for x in runs.tolist():
        op, k = x & 15, x >> 4
        cig.append(f"{k}{' M=XID'[op]}")
        if op == 2:
            same += k; cs.append(f":{k}"); i += k; j += k
        elif op == 3:
            for t in range(k):
                md.append(f"{same}{r[j + t]}"); same = 0
                cs.append(f"*{rl[j + t]}{ql[i + t]}")
            i += k; j += k
        elif op == 4:
            cs.append("+" + ql[i:i + k]); i += k
        else:
            md.append(f"{same}^{r[j:j + k]}"); same = 0
            cs.append("-" + rl[j:j + k]); j += k
    md.append(str(same))
    return "".join(cig), "".join(md), "".join(cs)


def host_path():
    t0 = time.perf_counter()
    res = cb.results()
    runs, off = cb.cigars(res["cigar_len"])
    t1 = time.perf_counter()
    st = host_stats(res, runs, off)
    t2 = time.perf_counter()
    strings = [host_strings(c, runs[int(off[c]):int(off[c + 1])], int(st["q_start"][c]), int(st["r_start"][c])) for c in range(n)]
    t3 = time.perf_counter()
    return dict(download_ms=(t1 - t0) * 1e3, numpy_stats_ms=(t2 - t1) * 1e3, python_strings_ms=(t3 - t2) * 1e3, end_to_end_ms=(t3 - t0) * 1e3,
                runs=int(len(runs))), st, strings


device_path(); host_path()   # untimed: the first use of the report's kernels and buffers
dev, hst = [], []
for _ in range(runs_timed):
    dev.append(device_path()); hst.append(host_path())
pick = lambda xs: sorted(xs, key=lambda x: x[0]["end_to_end_ms"])[len(xs) // 2]   # noqa: E731
(d, dst, dtext), (h, hstat, hstr) = pick(dev), pick(hst)
agree = all(np.array_equal(np.asarray(dst[k], dtype=np.float64), np.asarray(hstat[k], dtype=np.float64)) for k in dst) and set(dst) == set(hstat)
for k, (name, _) in enumerate(FORMATS):
    buf, off = dtext[name]
    joined = "".join(s[k] for s in hstr).encode("latin-1")
    agree = agree and buf.tobytes() == joined and np.array_equal(np.diff(off.astype(np.int64)), [len(s[k]) for s in hstr])
cb.close()
out["device"], out["host"] = d, h
out["end_to_end_ms_all"] = dict(device=[x[0]["end_to_end_ms"] for x in dev], host=[x[0]["end_to_end_ms"] for x in hst])
out["fills_ms"] = fills_ms
kernels = d["stats_kernels_ms"] + sum(d["text_kernels_ms"].values())
out["report_kernels_ms"] = kernels
out["report_kernels_over_fills"] = kernels / max(fills_ms, 1e-9)
out["stats_kernels_over_fills"] = d["stats_kernels_ms"] / max(fills_ms, 1e-9)
out["host_over_device_end_to_end"] = h["end_to_end_ms"] / d["end_to_end_ms"]
out["agree"] = bool(agree)
out["device_faster"] = bool(d["end_to_end_ms"] < h["end_to_end_ms"])   # the one bar
out["expectation_held"] = dict(end_to_end=bool(out["host_over_device_end_to_end"] >= 50), report_kernels=bool(out["report_kernels_over_fills"] < 0.25),
                               stats_kernels=bool(out["stats_kernels_over_fills"] < 0.1))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "chain_report_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if agree and out["device_faster"] else 1)
