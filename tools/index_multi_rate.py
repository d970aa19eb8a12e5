#!/usr/bin/env python3
"""What several sequences per index cost on the GPU, against the unchanged single-reference path of the same run.
  index:  the 3 Mbp random reference of tools/index_rate.py (k 15, w 10) built through ba_ref_index_create and through
          ba_ref_index_create_multi as 1, 24 and 3000 sequences of equal length: the three device times and the whole call
  fill:   the workload of tools/chaining_rate.py (raw 15-mer hits of 10 kbp reads against their reference stretches, plus noise) through
          AnchorChainer without a table and bounded by a table of one sequence: the fill's device time
Medians of three after one untimed pass, the variants taken in turn within every round. The one bar compares with the unchanged path of
the same run: the one-sequence create_multi build and the one-sequence bounded fill are each no slower than their unbounded counterparts
by more than the spread those counterparts show between their own three repetitions. Prints the figures and writes them to
profiles/index_multi_rate.json; exits 1 when a bar is missed.
usage: index_multi_rate.py [reference bases] [reads of the fill] [runs]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from block_aligner_amd import hip as H, synth   # noqa: E402

ref_len = int(sys.argv[1]) if len(sys.argv) > 1 else 3_000_000
n_reads = int(sys.argv[2]) if len(sys.argv) > 2 else 2000
runs_timed = int(sys.argv[3]) if len(sys.argv) > 3 else 3
K, W, NOISE = 15, 10, 0.25
P = (2, 1, 0, 64, 1000, 100, 2, 60, 2)   # tools/chaining_rate.py's
SPLITS = (1, 24, 3000)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


out = dict(reference_bases=ref_len, k=K, w=W, fill_reads=n_reads, runs=runs_timed,
           params=dict(zip("match_w drift_cost skip_cost lookback max_dist bandwidth max_chains min_score min_anchors".split(), P)),
           expectation="stated before the first run: one sequence through create_multi runs the kernels ba_ref_index_create runs, so its three "
                       "device times equal that call's within its own spread; 24 sequences likewise, within 10 % (24 more partial spans "
                       "of 2900); 3000 sequences of 1 kbp are 3000 short spans where one sequence has 2930 full ones, each found by a "
                       "lower bound over 3001 entries: the sketch within 1.5x of one sequence, sort and table unchanged but for the "
                       "entries the junctions cost; the whole call longer by the host's pack of 3 MB, under 1 ms; the bounded fill with a "
                       "table of one sequence within 5 % of the unbounded fill (one two-entry search per anchor, off the recurrence's "
                       "dependent chain)")

# ---- the index
rng = np.random.default_rng(4321)
ref = synth.rand_str(rng, ref_len, synth.DNA)


def build(parts):
    t0 = time.perf_counter()
    if parts is None:
        ix = H.RefIndex(K, W, ref)
    else:
        cut = np.linspace(0, ref_len, parts + 1).astype(np.uint64)
        ix = H.RefIndex.from_sequences(K, W, ref, cut[:-1], np.diff(cut).astype(np.uint32))
    wall = (time.perf_counter() - t0) * 1e3
    d = dict(ix.times(), build_ms=wall)
    c = ix.counts()
    ix.close()
    d["kernels_ms"] = d["sketch_ms"] + d["sort_ms"] + d["table_ms"]
    return d, int(c["n_entries"]), int(c["longest_run"])


def timed(fn, variants):
    """Every variant once untimed (the first use of the device, the allocator's first blocks of this size), then runs_timed rounds that
    take the variants in turn, so that whatever drifts during the run drifts under all of them -> per variant (medians, spreads, last)."""
    for v in variants:
        fn(v)
    got = [[] for _ in variants]
    for _ in range(runs_timed):
        for g, v in zip(got, variants):
            g.append(fn(v))
    res = []
    for g in got:
        keys = [k for k in g[0][0] if k.endswith("_ms")]
        res.append(({k: float(np.median([x[0][k] for x in g])) for k in keys},
                    {k: float(max(x[0][k] for x in g) - min(x[0][k] for x in g)) for k in keys}, g[-1]))
    return res


builds = timed(build, (None,) + SPLITS)
single, single_spread, last = builds[0]
out["index_single"] = dict(single, spread=single_spread, entries=last[1], longest_run=last[2])
say("single", out["index_single"])
for parts, (med, spread, last) in zip(SPLITS, builds[1:]):
    out[f"index_multi_{parts}"] = dict(med, spread=spread, entries=last[1], longest_run=last[2])
    say(parts, out[f"index_multi_{parts}"])
assert out["index_multi_1"]["entries"] == out["index_single"]["entries"]

# ---- the fill: the hits of tools/chaining_rate.py
rng = np.random.default_rng(1234)
n = n_reads
seqs = []
for c in range(n):
    read, rf = [], []
    for k in range(int(rng.integers(28, 40))):
        g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
        h = synth.mutate(rng, g, len(g) // 10, synth.DNA)
        a = synth.rand_str(rng, K, synth.DNA)
        read += [h, a]; rf += [g, a]
    g = synth.rand_str(rng, int(rng.integers(150, 450)), synth.DNA)
    read.append(synth.mutate(rng, g, len(g) // 10, synth.DNA)); rf.append(g)
    seqs += [np.concatenate(read), np.concatenate(rf)]
lens = np.array([len(s) for s in seqs], np.int64)
offs = np.concatenate([[0], np.cumsum(lens)[:-1]])
pool = np.concatenate(seqs)
code = np.zeros(256, np.uint64)
for i, b in enumerate(b"ACGT"):
    code[b] = i
two = code[pool]
kmer = np.zeros(len(pool) - K + 1, np.uint64)
for t in range(K):
    kmer |= two[t:len(pool) - K + 1 + t] << np.uint64(2 * t)
seq_of = np.repeat(np.arange(2 * n), lens)[:len(kmer)]
start = np.arange(len(kmer)) - offs[seq_of]
inside = start + K <= lens[seq_of]
key = (seq_of // 2).astype(np.uint64) << np.uint64(2 * K) | kmer
isq, isr = inside & (seq_of % 2 == 0), inside & (seq_of % 2 == 1)
rk, rpos = key[isr], start[isr]
o = np.argsort(rk, kind="stable")
rk, rpos = rk[o], rpos[o]
qk, qpos = key[isq], start[isq]
lo, hi = np.searchsorted(rk, qk, "left"), np.searchsorted(rk, qk, "right")
cnt = hi - lo
hit_q = np.repeat(qpos, cnt)
hit_p = np.repeat((qk >> np.uint64(2 * K)).astype(np.int64), cnt)
hit_r = rpos[np.repeat(lo, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
per = np.bincount(hit_p, minlength=n)
noise_p = np.repeat(np.arange(n), (per * NOISE).astype(np.int64))
noise_q = (rng.random(len(noise_p)) * (lens[0::2][noise_p] - K)).astype(np.int64)
noise_r = (rng.random(len(noise_p)) * (lens[1::2][noise_p] - K)).astype(np.int64)
hp, hq, hr = np.concatenate([hit_p, noise_p]), np.concatenate([hit_q, noise_q]), np.concatenate([hit_r, noise_r])
o = np.lexsort((hq, hr, hp))
hp, hq, hr = hp[o], hq[o].astype(np.uint32), hr[o].astype(np.uint32)
hl = np.full(len(hp), K, np.uint32)
first = np.concatenate([[0], np.cumsum(np.bincount(hp, minlength=n))]).astype(np.uint64)
out["fill_hits"] = int(len(hp))
table = [0, int(lens.max()) + 1]   # one sequence that holds every problem's reference positions


def fill(seq_start):
    ch = H.AnchorChainer(*P, first, hq, hr, hl, seq_start=seq_start)
    ch.run()
    t = ch.times()
    dp = ch.dp()
    ch.close()
    return dict(fill_ms=t["fill_ms"]), dp


(plain, plain_spread, plast), (bound, bound_spread, blast) = timed(fill, (None, table))
agree = all(np.array_equal(a, b) for a, b in zip(plast[1], blast[1]))
out["fill_unbounded"] = dict(plain, spread=plain_spread)
out["fill_bounded_one_sequence"] = dict(bound, spread=bound_spread, equals_unbounded=bool(agree))
say("fill", out["fill_unbounded"], out["fill_bounded_one_sequence"])

one, many = out["index_multi_1"], out["index_multi_3000"]
out["bar"] = dict(build=bool(one["kernels_ms"] - single["kernels_ms"] <= single_spread["kernels_ms"]),
                  fill=bool(bound["fill_ms"] - plain["fill_ms"] <= plain_spread["fill_ms"]))
out["expectation_held"] = dict(one_sequence=bool(abs(one["kernels_ms"] - single["kernels_ms"]) <= single_spread["kernels_ms"]),
                               twenty_four=bool(out["index_multi_24"]["kernels_ms"] <= 1.1 * one["kernels_ms"]),
                               three_thousand_sketch=bool(many["sketch_ms"] <= 1.5 * one["sketch_ms"]),
                               pack_under_1_ms=bool(one["build_ms"] - single["build_ms"] < 1.0),
                               bounded_fill=bool(bound["fill_ms"] <= 1.05 * plain["fill_ms"]))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "index_multi_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if agree and all(out["bar"].values()) else 1)
