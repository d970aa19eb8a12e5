#!/usr/bin/env python3
"""Mapping rate on the GPU with a reference index: one random reference of a few Mbp and reads of 10 kbp drawn from it with 5 % edits, half
of them from the minus strand, every read listed on both strands; k 15, w 10, no caps. From bytes to chains, twice in the same run:
  indexed: RefIndex (built once, timed on its own), then Seeder.indexed create (checks, upload of the reads), run (sketch, both sorts,
           lookup), AnchorChainer.from_seeder, run, results
  plain:   the parent API: Seeder with every problem's r the whole reference (its sketch is computed and stored once per problem), run,
           AnchorChainer.from_seeder, run, results; over as many of the problems as its memory allows
The hits of both paths must be equal. Then the chains of the indexed path go through candidate windows (margin 64) into a
ChainBatchAligner: its pack and fill times. Medians of three after one untimed pass. Prints the figures and writes them to
profiles/index_rate.json.
usage: index_rate.py [reads] [reference bases] [runs]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from block_aligner_amd import hip as H, scores, synth   # noqa: E402

n_reads = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
ref_len = int(sys.argv[2]) if len(sys.argv) > 2 else 3_000_000
runs_timed = int(sys.argv[3]) if len(sys.argv) > 3 else 3
K, W, NO_CAP, READ, MARGIN = 15, 10, 0xffffffff, 10000, 64
# match_w, drift_cost, skip_cost, lookback, max_dist, bandwidth, max_chains, min_score, min_anchors (tools/chaining_rate.py's)
P = (2, 1, 0, 64, 1000, 100, 2, 60, 2)
rng = np.random.default_rng(4321)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


# ---- the reference and the reads
ref = synth.rand_str(rng, ref_len, synth.DNA)
COMP = np.arange(256, dtype=np.uint8)
for a, b in zip(b"ACGT", b"TGCA"):
    COMP[a] = b
reads, origin = [], []
for i in range(n_reads):
    at = int(rng.integers(0, ref_len - READ))
    read = synth.mutate(rng, ref[at:at + READ], READ // 20, synth.DNA)
    if i % 2:
        read = COMP[read[::-1]]
    reads.append(read)
    origin.append((at, at + READ, i % 2))
lens = np.repeat(np.array([len(r) for r in reads], np.int64), 2)                     # every read on both strands: problems 2 i and 2 i + 1
offs = np.repeat(np.concatenate([[0], np.cumsum([len(r) for r in reads])[:-1]]), 2)
read_pool = np.concatenate(reads)
pool = np.concatenate([read_pool, ref, np.zeros(8, np.uint8)])                       # the reference behind the reads: the plain path and the chain batch
n = 2 * n_reads
q_off, q_len = offs.astype(np.uint64), lens.astype(np.uint32)
strand = np.tile(np.array([0, 1], np.uint8), n_reads)
r_off, r_len = np.full(n, len(read_pool), np.uint64), np.full(n, ref_len, np.uint32)

out = dict(reads=n_reads, problems=n, read_bases=int(len(read_pool)), reference_bases=ref_len, k=K, w=W, max_occ=NO_CAP, max_ref_occ=NO_CAP, margin=MARGIN,
           params=dict(zip("match_w drift_cost skip_cost lookback max_dist bandwidth max_chains min_score min_anchors".split(), P)),
           expectation="stated before the first run: the indexed path end to end (Seeder.indexed create, run, from_seeder, run, results) at "
                       "least 10 times faster than the plain path over the same problems; the three parts of the index build together under "
                       "5 ms for 3 Mbp, the sketch the longest of them; the indexed seeder's three times together under 20 ms for 4000 "
                       "problems, the lookup the longest of them; the windowed chain batch packs less than 1/100 of the bytes that "
                       "whole-reference ends would take")


def chain(sd):
    ch = H.AnchorChainer.from_seeder(*P, sd)
    ch.run()
    return ch, ch.results()


def indexed(ix):
    t0 = time.perf_counter()
    sd = H.Seeder.indexed(ix, NO_CAP, NO_CAP, read_pool, q_off, q_len, strand)
    sd.run()
    t1 = time.perf_counter()
    ch, res = chain(sd)
    t2 = time.perf_counter()
    tt, c = sd.times(), sd.counts()
    hits = sd.results()
    sd.close()
    return dict(sketch_ms=tt["sketch_ms"], sort_ms=tt["sort_ms"], lookup_ms=tt["match_ms"], seeder_ms=(t1 - t0) * 1e3, end_to_end_ms=(t2 - t0) * 1e3,
                hits=int(c["n_hits"]), q_seeds=int(c["n_q_seeds"]), longest_problem=int(c["hits_per_problem"].max())), hits, res, ch


def plain(m):
    """The first m problems through the parent commit's API."""
    t0 = time.perf_counter()
    sd = H.Seeder(K, W, NO_CAP, pool, q_off[:m], q_len[:m], r_off[:m], r_len[:m], strand[:m])
    sd.run()
    t1 = time.perf_counter()
    ch, res = chain(sd)
    t2 = time.perf_counter()
    tt, c = sd.times(), sd.counts()
    hits = sd.results()
    sd.close(); ch.close()
    return dict(sketch_ms=tt["sketch_ms"], sort_ms=tt["sort_ms"], match_ms=tt["match_ms"], seeder_ms=(t1 - t0) * 1e3, end_to_end_ms=(t2 - t0) * 1e3,
                r_seeds=int(c["n_r_seeds"])), hits, res


def median(ds):
    return {k: float(np.median([d[k] for d in ds])) for k in ds[0] if k.endswith("_ms")}


# ---- the index build
H.RefIndex(K, W, ref).close()   # (the first use of the device: context, code objects, the allocator's first blocks)
builds = []
for _ in range(runs_timed):
    t0 = time.perf_counter()
    ix = H.RefIndex(K, W, ref)
    wall = (time.perf_counter() - t0) * 1e3
    builds.append(dict(ix.times(), build_ms=wall))
    c = ix.counts()
    if len(builds) < runs_timed:
        ix.close()
out["index"] = dict(median(builds), entries=int(c["n_entries"]), longest_run=int(c["longest_run"]))
say("index", out["index"])

# ---- the indexed path
indexed(ix)[3].close()
got = []
for _ in range(runs_timed):
    got.append(indexed(ix))
    if len(got) < runs_timed:
        got[-1][3].close()
d, hits, res, ch = got[-1]
out["indexed"] = dict(median([g[0] for g in got]), hits=d["hits"], q_seeds=d["q_seeds"], longest_problem=d["longest_problem"], chains=int(len(res["chain_problem"])))
say("indexed", out["indexed"])

# ---- the plain path: as many of the problems as fit
m = n
while True:
    try:
        plain(m)
        break
    except RuntimeError as e:
        if "hipMalloc" not in str(e) or m < 8:
            raise
        say(f"plain: {m} problems do not fit ({e}); halving")
        m //= 2
pgot = [plain(m) for _ in range(runs_timed)]
pd, phits, pres = pgot[-1]
first = hits[0]
end = int(first[m])
agree = np.array_equal(phits[0], first[:m + 1]) and all(np.array_equal(a, b[:end]) for a, b in zip(phits[1:4], hits[1:4]))
assert agree, "the indexed seeder's hits differ from the plain seeder's"
out["plain"] = dict(median([g[0] for g in pgot]), problems=m, r_seeds=pd["r_seeds"], hits_agree=bool(agree))
say("plain", out["plain"])
scale = n / m   # (the plain path's time grows with its problems: every one brings a reference to sketch and to walk)
if m < n:       # the same m problems through the indexed path, for the comparison
    q_off, q_len, strand = q_off[:m], q_len[:m], strand[:m]
    igot = [indexed(ix) for _ in range(runs_timed + 1)][1:]
    for g in igot:
        g[3].close()
    out["indexed_same_problems"] = median([g[0] for g in igot])
    same = out["indexed_same_problems"]["end_to_end_ms"]
else:
    same = out["indexed"]["end_to_end_ms"]
out["plain_over_indexed_end_to_end"] = out["plain"]["end_to_end_ms"] / same
out["indexed_faster_than_plain"] = bool(out["plain_over_indexed_end_to_end"] > 1)

# ---- the chains of the indexed path through candidate windows into a chain batch
m_nuc = scores.NucMatrix.new_simple(2, -3)
full_off, full_len, full_strand = offs.astype(np.uint64), lens.astype(np.uint32), np.tile(np.array([0, 1], np.uint8), n_reads)
args = ch.chain_batch_args(pool, full_off, full_len, r_off, r_len, full_strand, margin=MARGIN)
shift = ch.last_window_shift
cbs = []
for _ in range(runs_timed + 1):
    t0 = time.perf_counter()
    cb = H.ChainBatchAligner(m_nuc, (-5, -1), (32, 256), 100, H.X_DROP | H.TRACE, *args)
    ms = cb.run()
    cres = cb.results()
    wall = (time.perf_counter() - t0) * 1e3
    cbs.append(dict(cb.times(), fills_ms=ms, chain_batch_ms=wall))
    cb.close()
cp, rank = res["chain_problem"], res["chain_rank"]
placed = 0
for c in np.nonzero(rank == 0)[0]:
    i, s = int(cp[c]) // 2, int(cp[c]) % 2
    lo, hi = int(cres["r_start"][c]) + int(shift[c]), int(cres["r_end"][c]) + int(shift[c])
    placed += s == origin[i][2] and lo < origin[i][1] and origin[i][0] < hi
window_bytes = int(args[4].astype(np.int64).sum())
out["chain_batch"] = dict(median(cbs[1:]), chains=int(len(cp)), window_bytes=window_bytes, whole_reference_bytes=int(len(cp)) * ref_len,
                          reads_placed_on_their_origin=int(placed), failed=int((cres["status"] != 0).sum()))
ch.close(); ix.close()
say("chain_batch", out["chain_batch"])

b, s = out["index"], out["indexed"]
out["expectation_held"] = dict(end_to_end=bool(out["plain_over_indexed_end_to_end"] >= 10),
                               build=bool(b["sketch_ms"] + b["sort_ms"] + b["table_ms"] < 5 * ref_len / 3e6 and b["sketch_ms"] >= max(b["sort_ms"], b["table_ms"])),
                               seeder=bool((s["sketch_ms"] + s["sort_ms"] + s["lookup_ms"]) * 4000 / n < 20 and s["lookup_ms"] >= max(s["sketch_ms"], s["sort_ms"])),
                               windows=bool(window_bytes * 100 < out["chain_batch"]["whole_reference_bytes"]))
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "index_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if agree and out["indexed_faster_than_plain"] else 1)
