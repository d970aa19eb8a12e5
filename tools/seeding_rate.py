#!/usr/bin/env python3
"""Seeding rate on the GPU: the reads of tools/chaining_rate.py (10 kbp DNA reads against their reference stretch) from bytes to chains, twice:
with k 15, w 1 and no cap -- every shared 15-mer of a read and its reference is a hit: the device's hits must equal that tool's NumPy "true
hits" exactly -- and with k 15, w 10.
  seeded:  Seeder create (checks, upload of the bytes), run (sketch, sort, match), AnchorChainer.from_seeder (the hits stay on the device),
           run, results
  host:    the same hits in NumPy (for w 1 the code of tools/chaining_rate.py, for w 10 the minimizers of the whole pool at once), sorted on
           the host, then AnchorChainer from the host arrays (checks, upload of the hits), run, results
Prints the three device times of the seeder and both paths end to end, checks that hits and chains are equal, and writes the same to
profiles/seeding_rate.json.
usage: seeding_rate.py [reads] [runs]"""
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
K, NO_CAP = 15, 0xffffffff
# match_w, drift_cost, skip_cost, lookback, max_dist, bandwidth, max_chains, min_score, min_anchors (tools/chaining_rate.py's)
P = (2, 1, 0, 64, 1000, 100, 2, 60, 2)
rng = np.random.default_rng(1234)

# ---- the reads of tools/chaining_rate.py
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
q_off, r_off = offs[0::2].astype(np.uint64), offs[1::2].astype(np.uint64)
q_len, r_len = lens[0::2].astype(np.uint32), lens[1::2].astype(np.uint32)

out = dict(reads=n, bases=int(len(pool)), k=K, max_occ=NO_CAP,
           params=dict(zip("match_w drift_cost skip_cost lookback max_dist bandwidth max_chains min_score min_anchors".split(), P)),
           expectation="stated before the first run: the seeded path end to end (Seeder create, run, from_seeder, run, results) at least 20 "
                       "times faster than the host path (NumPy seeding, AnchorChainer from host arrays) for w 1 and for w 10; the seeder's "
                       "three kernels together under 30 ms per 2000 reads at w 1 and under 10 ms at w 10; the sort the longest of the three "
                       "at w 1 (queries of 10 000 entries take the global-memory network), the sketch the longest at w 10")


# ---- seeding on the host
def true_hits():
    """Every shared 15-mer of a read and its reference, as tools/chaining_rate.py computes its "true hits" -> (problem, q, r), unsorted."""
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
    return join(key[isq], start[isq], key[isr], start[isr])


def join(qk, qpos, rk, rpos):
    """Every pair of a query entry and a reference entry with the same (problem, code) key -> (problem, q, r), unsorted."""
    o = np.argsort(rk, kind="stable")
    rk, rpos = rk[o], rpos[o]
    lo, hi = np.searchsorted(rk, qk, "left"), np.searchsorted(rk, qk, "right")
    cnt = hi - lo
    hit_q = np.repeat(qpos, cnt)
    hit_p = np.repeat((qk >> np.uint64(2 * K)).astype(np.int64), cnt)
    hit_r = rpos[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
    return hit_p, hit_q, hit_r


def minimizer_hits(w):
    """The rule of INTEGRATION.md, "Seeding", over the whole pool at once (the sequences hold ACGT only and are longer than k + w; no cap)."""
    code = np.zeros(256, np.uint64)
    for i, b in enumerate(b"ACGT"):
        code[b] = i
    two = code[pool]
    nk = len(pool) - K + 1
    kmer = np.zeros(nk, np.uint64)
    for t in range(K):
        kmer = kmer << np.uint64(2) | two[t:nk + t]
    x = kmer ^ np.uint64(0x9e3779b9)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85ebca6b)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xc2b2ae35)) & np.uint64(0xffffffff)
    x ^= x >> np.uint64(16)
    seq_of = np.repeat(np.arange(2 * n), lens)[:nk]
    start = np.arange(nk) - offs[seq_of]
    inside = start + K <= lens[seq_of]
    order_key = x << np.uint64(32) | np.arange(nk, dtype=np.uint64)      # (the position in the pool orders like the position in the sequence)
    order_key[~inside] = np.uint64(0xffffffffffffffff)
    if w > 1:
        mins = np.lib.stride_tricks.sliding_window_view(order_key, w).min(axis=1)
        real = inside[:nk - w + 1] & inside[w - 1:] & (seq_of[:nk - w + 1] == seq_of[w - 1:])   # a window lies within one sequence
        sel = np.unique(mins[real] & np.uint64(0xffffffff)).astype(np.int64)
    else:
        sel = np.nonzero(inside)[0]
    key = (seq_of[sel] // 2).astype(np.uint64) << np.uint64(2 * K) | kmer[sel]
    isq = seq_of[sel] % 2 == 0
    return join(key[isq], start[sel][isq], key[~isq], start[sel][~isq])


def host(w):
    t0 = time.perf_counter()
    hp, hq, hr = true_hits() if w == 1 else minimizer_hits(w)
    o = np.lexsort((hq, hr, hp))                              # (all hits have K columns: sorted by start = sorted by end)
    hp, hq, hr = hp[o], hq[o].astype(np.uint32), hr[o].astype(np.uint32)
    hl = np.full(len(hp), K, np.uint32)
    first = np.concatenate([[0], np.cumsum(np.bincount(hp, minlength=n))]).astype(np.uint64)
    t1 = time.perf_counter()
    ch = H.AnchorChainer(*P, first, hq, hr, hl)
    ch.run()
    res = ch.results()
    t2 = time.perf_counter()
    ch.close()
    return dict(seeding_ms=(t1 - t0) * 1e3, chaining_ms=(t2 - t1) * 1e3, end_to_end_ms=(t2 - t0) * 1e3), (first, hq, hr), res


def seeded(w):
    t0 = time.perf_counter()
    sd = H.Seeder(K, w, NO_CAP, pool, q_off, q_len, r_off, r_len)
    sd.run()
    t1 = time.perf_counter()
    ch = H.AnchorChainer.from_seeder(*P, sd)
    ch.run()
    res = ch.results()
    t2 = time.perf_counter()
    tt = sd.times()
    ct = ch.times()
    c = sd.counts()
    hits = sd.results()
    sd.close(); ch.close()
    return dict(sketch_ms=tt["sketch_ms"], sort_ms=tt["sort_ms"], match_ms=tt["match_ms"], fill_ms=ct["fill_ms"], pick_ms=ct["pick_ms"],
                gather_ms=ct["gather_ms"], seeder_ms=(t1 - t0) * 1e3, end_to_end_ms=(t2 - t0) * 1e3, hits=int(c["n_hits"]),
                q_seeds=int(c["n_q_seeds"]), r_seeds=int(c["n_r_seeds"]), longest_problem=int(c["hits_per_problem"].max())), hits, res


ok = True
seeded(1)   # (the first use of the device: context, code objects, the allocator's first blocks)
for w in (1, 10):
    got = [seeded(w) for _ in range(runs_timed)]
    med = {k: float(np.median([g[0][k] for g in got])) for k in got[0][0] if k.endswith("_ms")}
    d, (first, hq, hr, _, _), res = sorted(got, key=lambda g: g[0]["end_to_end_ms"])[runs_timed // 2]
    host(w)   # (untimed, as for the seeded path)
    hgot = [host(w) for _ in range(runs_timed)]
    _, (hfirst, hhq, hhr), hres = hgot[0]
    h = {k: float(np.median([g[0][k] for g in hgot])) for k in hgot[0][0]}
    agree = np.array_equal(first, hfirst) and np.array_equal(hq, hhq) and np.array_equal(hr, hhr)
    assert agree, f"w {w}: the device's hits differ from the host's"   # (w 1: tools/chaining_rate.py's true hits, before its noise)
    chains_agree = all(np.array_equal(res[k], hres[k]) for k in res)
    ok = ok and agree and chains_agree
    kernels = {k: med[k] for k in ("sketch_ms", "sort_ms", "match_ms")}
    out[f"w{w}"] = dict(w=w, hits=int(d["hits"]), q_seeds=int(d["q_seeds"]), r_seeds=int(d["r_seeds"]), longest_problem=int(d["longest_problem"]),
                        seeded=med, host=h, hits_agree=bool(agree), chains_agree=bool(chains_agree),
                        chains=int(len(res["chain_problem"])), host_over_seeded_end_to_end=h["end_to_end_ms"] / med["end_to_end_ms"],
                        longest_kernel=max(kernels, key=kernels.get))
out["seeded_faster_than_host"] = bool(all(out[f"w{w}"]["host_over_seeded_end_to_end"] > 1 for w in (1, 10)))
ksum = lambda w: sum(out[f"w{w}"]["seeded"][k] for k in ("sketch_ms", "sort_ms", "match_ms")) * 2000 / n   # noqa: E731
out["expectation_held"] = dict(end_to_end=bool(all(out[f"w{w}"]["host_over_seeded_end_to_end"] >= 20 for w in (1, 10))),
                               kernels=bool(ksum(1) < 30 and ksum(10) < 10),
                               longest=bool(out["w1"]["longest_kernel"] == "sort_ms" and out["w10"]["longest_kernel"] == "sketch_ms"))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "seeding_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if ok and out["seeded_faster_than_host"] else 1)
