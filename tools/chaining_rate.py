#!/usr/bin/env python3
"""Anchor-chaining rate on the GPU: the reads of tools/chain_rate.py (10 kbp DNA reads against their reference stretch, an exact 15-base anchor
every few hundred bases, ~10 % edits between them) as a mapper sees them before chaining: every shared 15-mer of a read and its reference as
a raw hit -- overlapping wherever more than 15 bases survived the edits --, plus uniformly placed noise hits, sorted by (reference end, query
end) per read.
  device:  AnchorChainer -- create (checks, upload), run (fill, pick, gather), results
  host:    the same rule in NumPy: the fill with the look-back vectorised (over the H candidates of an anchor, and over the reads), the
           picking and the output anchors per read
Prints the device times per kernel and end to end for both, checks that chains and anchors are equal, and writes the same to
profiles/chaining_rate.json.
usage: chaining_rate.py [reads] [runs]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from block_aligner_amd import hip as H, synth   # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
runs_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 3
K, NOISE = 15, 0.25
# match_w, drift_cost, skip_cost, lookback, max_dist, bandwidth, max_chains, min_score, min_anchors
P = (2, 1, 0, 64, 1000, 100, 2, 60, 2)
rng = np.random.default_rng(1234)

# ---- the reads of tools/chain_rate.py
seqs = []
for c in range(n):
    read, ref = [], []
    for k in range(int(rng.integers(28, 40))):
        g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
        h = synth.mutate(rng, g, len(g) // 10, synth.DNA)
        a = synth.rand_str(rng, K, synth.DNA)
        read += [h, a]; ref += [g, a]
    g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
    read.append(synth.mutate(rng, g, len(g) // 10, synth.DNA)); ref.append(g)
    seqs += [np.concatenate(read), np.concatenate(ref)]
lens = np.array([len(s) for s in seqs], np.int64)
offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
pool = np.concatenate(seqs)

# ---- seeding on the host (not what is measured): every shared 15-mer of a read and its reference
t0 = time.perf_counter()
code = np.zeros(256, np.uint64)
for i, b in enumerate(b"ACGT"):
    code[b] = i
two = code[pool]
kmer = np.zeros(len(pool) - K + 1, np.uint64)
for t in range(K):
    kmer |= two[t:len(pool) - K + 1 + t] << np.uint64(2 * t)
seq_of = np.repeat(np.arange(2 * n), lens)[:len(kmer)]
start = np.arange(len(kmer)) - offs[seq_of]
inside = start + K <= lens[seq_of]                       # (a window must not run into the next sequence)
key = (seq_of // 2).astype(np.uint64) << np.uint64(2 * K) | kmer
isq = inside & (seq_of % 2 == 0)
isr = inside & (seq_of % 2 == 1)
rk, rpos = key[isr], start[isr]
o = np.argsort(rk, kind="stable")
rk, rpos = rk[o], rpos[o]
qk, qpos = key[isq], start[isq]
lo, hi = np.searchsorted(rk, qk, "left"), np.searchsorted(rk, qk, "right")
cnt = hi - lo
hit_q = np.repeat(qpos, cnt)
hit_p = np.repeat((qk >> np.uint64(2 * K)).astype(np.int64), cnt)
hit_r = rpos[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
true_hits = len(hit_q)
per = np.bincount(hit_p, minlength=n)
noise_n = (per * NOISE).astype(np.int64)
noise_p = np.repeat(np.arange(n), noise_n)
noise_q = (rng.random(len(noise_p)) * (lens[0::2][noise_p] - K)).astype(np.int64)
noise_r = (rng.random(len(noise_p)) * (lens[1::2][noise_p] - K)).astype(np.int64)
hp, hq, hr = np.concatenate([hit_p, noise_p]), np.concatenate([hit_q, noise_q]), np.concatenate([hit_r, noise_r])
o = np.lexsort((hq, hr, hp))                              # (all hits have K columns: sorted by start = sorted by end)
hp, hq, hr = hp[o], hq[o].astype(np.uint32), hr[o].astype(np.uint32)
hl = np.full(len(hp), K, np.uint32)
first = np.concatenate([[0], np.cumsum(np.bincount(hp, minlength=n))]).astype(np.uint64)
seed_ms = (time.perf_counter() - t0) * 1e3
out = dict(reads=n, hits=int(len(hp)), true_hits=int(true_hits), noise_hits=int(len(noise_p)), longest_problem=int(np.diff(first).max()),
           params=dict(zip("match_w drift_cost skip_cost lookback max_dist bandwidth max_chains min_score min_anchors".split(), P)),
           host_seeding_ms=seed_ms,
           expectation="stated before the first run: the device end to end (create, run, results) at least 20 times faster than the NumPy "
                       "host rule; the three kernels together under 5 ms per 2000 reads; the fill the longest of the three")


# ---- the device
def device():
    t0 = time.perf_counter()
    ch = H.AnchorChainer(*P, first, hq, hr, hl)
    ch.run()
    res = ch.results()
    e2e = (time.perf_counter() - t0) * 1e3
    tt = []
    for _ in range(runs_timed):
        ch.run(); tt.append(ch.times())
    med = lambda k: float(np.median([t[k] for t in tt]))   # noqa: E731
    f, pred = ch.dp()
    ch.close()
    return dict(fill_ms=med("fill_ms"), pick_ms=med("pick_ms"), gather_ms=med("gather_ms"), end_to_end_ms=e2e), res, f, pred


# ---- the host: the same rule
def host():
    t0 = time.perf_counter()
    mw, dc, sc, Hh, md, bw, mc, ms, ma = P
    cntp = np.diff(first).astype(np.int64)
    W = int(cntp.max())
    idx = first[:-1].astype(np.int64)[:, None] + np.arange(W)[None, :]
    ok = np.arange(W)[None, :] < cntp[:, None]
    idx = np.where(ok, idx, 0)
    L = np.where(ok, hl[idx].astype(np.int64), 0)
    qe = np.where(ok, hq[idx].astype(np.int64) + L, -(1 << 40))   # (padding is admissible to nothing)
    re = np.where(ok, hr[idx].astype(np.int64) + L, -(1 << 40))
    f = np.zeros((n, W), np.int64); pred = np.full((n, W), -1, np.int64); gain = L.copy()
    rows = np.arange(n)
    for i in range(W):
        lo_j = max(0, i - Hh)
        best = mw * L[:, i]
        if i > lo_j:
            dq = qe[:, i, None] - qe[:, lo_j:i]; dr = re[:, i, None] - re[:, lo_j:i]
            drift = np.abs(dq - dr); low = np.minimum(dq, dr)
            g = np.minimum(L[:, i, None], low)
            v = f[:, lo_j:i] + mw * g - dc * drift - sc * (low - g)
            v = np.where((dq > 0) & (dr > 0) & (dq <= md) & (dr <= md) & (drift <= bw), v, -(1 << 60))
            rev = v[:, ::-1]                                   # nearest first: argmax takes the first of equals
            k = np.argmax(rev, axis=1)
            vb = rev[rows, k]
            take = vb > best                                   # "none" wins a tie
            j = i - 1 - k
            best = np.where(take, vb, best)
            pred[:, i] = np.where(take, j, -1)
            gain[:, i] = np.where(take, g[rows, j - lo_j], L[:, i])
        f[:, i] = best
    t_fill = (time.perf_counter() - t0) * 1e3
    chains = []   # (problem, rank, score, [(q, r, len, src)])
    for p in range(n):
        c = int(cntp[p])
        fp, pp, gp = f[p, :c], pred[p, :c].tolist(), gain[p, :c]
        used = np.zeros(c, bool)
        rank = 0
        for _ in range(mc):
            if used.all():
                break
            e = int(np.argmax(np.where(used, -(1 << 60), fp)))
            if fp[e] < ms:
                break
            path, k = [], e
            while k != -1 and not used[k]:
                path.append(k); used[k] = True; k = pp[k]
            score = int(fp[e]) if k == -1 else int(fp[e] - fp[k])
            if score >= ms and len(path) >= ma:
                path.reverse()
                chains.append((p, rank, score, [(int(qe[p, x] - gp[x]), int(re[p, x] - gp[x]), int(gp[x]), x) for x in path]))
                rank += 1
    e2e = (time.perf_counter() - t0) * 1e3
    return dict(fill_ms=t_fill, pick_ms=e2e - t_fill, end_to_end_ms=e2e), chains, f, pred, ok


device()   # (the first use of the device: context, code objects, the allocator's first blocks)
dev = sorted([device() for _ in range(runs_timed)], key=lambda x: x[0]["end_to_end_ms"])[runs_timed // 2]
d, res, df, dpred = dev
h, chains, hf, hpred, ok = host()
out["device"], out["host"] = d, h
agree = np.array_equal(df, hf[ok]) and np.array_equal(dpred, hpred[ok])
agree = agree and len(chains) == len(res["chain_problem"])
if agree:
    agree = (res["chain_problem"].tolist() == [c[0] for c in chains] and res["chain_rank"].tolist() == [c[1] for c in chains] and
             res["chain_score"].tolist() == [c[2] for c in chains] and
             res["anchor_first"].tolist() == np.concatenate([[0], np.cumsum([len(c[3]) for c in chains])]).tolist() and
             list(zip(res["q_anchor"].tolist(), res["r_anchor"].tolist(), res["anchor_len"].tolist(), res["anchor_src"].tolist())) ==
             [a for c in chains for a in c[3]])
out["agree"] = bool(agree)
out["chains"], out["chain_anchors"] = int(len(res["chain_problem"])), int(len(res["q_anchor"]))
out["host_over_device_end_to_end"] = h["end_to_end_ms"] / d["end_to_end_ms"]
out["expectation_held"] = dict(end_to_end=bool(out["host_over_device_end_to_end"] >= 20),
                               kernels=bool((d["fill_ms"] + d["pick_ms"] + d["gather_ms"]) * 2000 / n < 5),
                               fill_longest=bool(d["fill_ms"] > max(d["pick_ms"], d["gather_ms"])))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "chaining_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if agree else 1)
