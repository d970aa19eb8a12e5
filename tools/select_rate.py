#!/usr/bin/env python3
"""Read-level selection on the GPU against the same rule on the host, over the workload of tools/index_rate.py: one random reference of a
few Mbp and reads of 10 kbp drawn from it with 5 % edits, half of them from the minus strand, every read listed on both strands; seeded
against a RefIndex, chained, cut to candidate windows and aligned by a ChainBatchAligner. Then, both in the same process:
  device: Selector.from_chain_batch (the batch's results stay on the device), run, results
  host:   ChainBatchAligner.results() downloaded, and the rule of INTEGRATION.md, "Selecting a read's alignments", in NumPy / Python:
          one lexsort for grouping and ranking, then the sweep read by read
The outputs of both paths must be equal. Medians of three after one untimed pass of each. Prints the figures and writes them to
profiles/select_rate.json.
usage: select_rate.py [reads] [reference bases] [runs]"""
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
P = (2, 1, 0, 64, 1000, 100, 2, 60, 2)   # the chainer's parameters of tools/index_rate.py
# mask_permille, sec_permille, max_secondary, mapq_max, full_support, min_score: minimap2's defaults where it has a counterpart
S = (500, 800, 5, 60, 10, 40)
rng = np.random.default_rng(4321)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


# ---- the reference and the reads (as tools/index_rate.py draws them)
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
    origin.append(i % 2)
lens = np.repeat(np.array([len(r) for r in reads], np.int64), 2)                     # every read on both strands: problems 2 i and 2 i + 1
offs = np.repeat(np.concatenate([[0], np.cumsum([len(r) for r in reads])[:-1]]), 2)
read_pool = np.concatenate(reads)
pool = np.concatenate([read_pool, ref, np.zeros(8, np.uint8)])
n = 2 * n_reads
q_off, q_len = offs.astype(np.uint64), lens.astype(np.uint32)
strand = np.tile(np.array([0, 1], np.uint8), n_reads)
r_off, r_len = np.full(n, len(read_pool), np.uint64), np.full(n, ref_len, np.uint32)

out = dict(reads=n_reads, problems=n, reference_bases=ref_len, k=K, w=W, margin=MARGIN,
           select=dict(zip("mask_permille sec_permille max_secondary mapq_max full_support min_score".split(), S)),
           expectation="stated before the first run: the device path end to end (Selector.from_chain_batch, run, results) faster than the host "
                       "path of the same run (ChainBatchAligner.results() and the rule in NumPy / Python); the three kernel times together "
                       "under 0.5 ms for these candidates, the marking the longest of them, and together below the chain batch's two fills")

# ---- from bytes to alignments
ix = H.RefIndex(K, W, ref)
sd = H.Seeder.indexed(ix, NO_CAP, NO_CAP, read_pool, q_off, q_len, strand)
sd.run()
ch = H.AnchorChainer.from_seeder(*P, sd)
ch.run()
sd.close(); ix.close()
chains = ch.results()
cb = H.ChainBatchAligner(scores.NucMatrix.new_simple(2, -3), (-5, -1), (32, 256), 100, H.X_DROP | H.TRACE,
                         *ch.chain_batch_args(pool, q_off, q_len, r_off, r_len, strand, margin=MARGIN))
fills_ms = cb.run()
cp = chains["chain_problem"]
read_of_chain = (cp // 2).astype(np.uint32)
support = np.diff(chains["anchor_first"].astype(np.int64)).astype(np.uint32)
c_len, c_strand = q_len[cp], strand[cp]
out["chains"] = int(len(cp))
out["chain_batch"] = dict(cb.times(), fills_ms=fills_ms)
say("chains", out["chains"], out["chain_batch"])


def device():
    t0 = time.perf_counter()
    sel = H.Selector.from_chain_batch(*S, cb, read_of_chain, support, n_reads)
    t1 = time.perf_counter()
    sel.run()
    t2 = time.perf_counter()
    res = sel.results()
    t3 = time.perf_counter()
    tt = sel.times()
    sel.close()
    return dict(tt, create_ms=(t1 - t0) * 1e3, run_ms=(t2 - t1) * 1e3, results_ms=(t3 - t2) * 1e3, end_to_end_ms=(t3 - t0) * 1e3), res


def host():
    """The rule over the downloaded results: cls, mapq, parent, rank, sub_score, kept_first, kept, kept_per_read."""
    t0 = time.perf_counter()
    r = cb.results()
    t1 = time.perf_counter()
    mask, sec, max_sec, mapq_max, full, min_score = S
    nc = len(cp)
    qs, qe, score = r["q_start"].astype(np.int64), r["q_end"].astype(np.int64), r["score"].astype(np.int64)
    ql, minus = c_len.astype(np.int64), c_strand.astype(bool)
    a, b = np.where(minus, ql - qe, qs), np.where(minus, ql - qs, qe)
    ok = ((r["status"] & H.STATS_FAILED_BITS) == 0) & (score >= min_score) & (b > a)
    cls, mapq = np.full(nc, H.SEL_EXCLUDED, np.uint8), np.zeros(nc, np.uint8)
    parent, rank, sub_score = np.full(nc, H.SEL_NONE, np.uint32), np.full(nc, H.SEL_NONE, np.uint32), np.zeros(nc, np.int32)
    idx = np.nonzero(ok)[0]
    idx = idx[np.lexsort((idx, -score[idx], read_of_chain[idx]))]   # by read, score descending, index ascending
    bounds = np.searchsorted(read_of_chain[idx], np.arange(n_reads + 1))
    kept, kept_per_read = [], np.zeros(n_reads, np.uint32)
    al, bl, sl, ul = a.tolist(), b.tolist(), score.tolist(), np.minimum(support, full).tolist()
    for rd in range(n_reads):
        heads, sub, secondaries, before = [], {}, 0, len(kept)
        for i, c in enumerate(idx[bounds[rd]:bounds[rd + 1]].tolist()):
            rank[c] = i
            found = None
            for h in heads:
                ov = min(bl[c], bl[h]) - max(al[c], al[h])
                if ov > 0 and 1000 * ov >= mask * min(bl[c] - al[c], bl[h] - al[h]):
                    found = h
                    break
            if found is None:
                heads.append(c); sub[c] = 0; parent[c] = c
                cls[c] = H.SEL_PRIMARY if i == 0 else H.SEL_SUPPLEMENTARY
                kept.append(c)
                continue
            parent[c] = found
            sub[found] = max(sub[found], sl[c])
            if 1000 * sl[c] >= sec * sl[found] and secondaries < max_sec:
                cls[c] = H.SEL_SECONDARY; secondaries += 1
                kept.append(c)
            else:
                cls[c] = H.SEL_DROPPED
        for h in heads:
            mapq[h] = (mapq_max * (sl[h] - sub[h]) * ul[h]) // (sl[h] * full)
            sub_score[h] = sub[h]
        kept_per_read[rd] = len(kept) - before
    res = dict(cls=cls, mapq=mapq, parent=parent, rank=rank, sub_score=sub_score,
               kept_first=np.concatenate([[0], np.cumsum(kept_per_read, dtype=np.uint64)]).astype(np.uint64), kept=np.array(kept, np.uint32),
               kept_per_read=kept_per_read)
    t2 = time.perf_counter()
    return dict(download_ms=(t1 - t0) * 1e3, rule_ms=(t2 - t1) * 1e3, end_to_end_ms=(t2 - t0) * 1e3), res


def median(ds):
    return {k: float(np.median([d[k] for d in ds])) for k in ds[0]}


device(); host()   # one untimed pass of each
dev = [device() for _ in range(runs_timed)]
hst = [host() for _ in range(runs_timed)]
dres, hres = dev[-1][1], hst[-1][1]
agree = all(np.array_equal(dres[k], hres[k]) for k in hres)
assert agree, "the device's selection differs from the host's: " + ", ".join(k for k in hres if not np.array_equal(dres[k], hres[k]))
on_origin = sum(int(c_strand[c]) == origin[int(read_of_chain[c])] for c in np.nonzero(dres["cls"] == H.SEL_PRIMARY)[0].tolist())
out["device"], out["host"] = median([d[0] for d in dev]), median([h[0] for h in hst])
out["classes"] = np.bincount(dres["cls"], minlength=5).tolist()
out["kept"] = int(len(dres["kept"]))
out["primaries_on_their_origin_strand"] = int(on_origin)
out["outputs_agree"] = bool(agree)
out["host_over_device_end_to_end"] = out["host"]["end_to_end_ms"] / out["device"]["end_to_end_ms"]
out["device_faster_than_host"] = bool(out["host_over_device_end_to_end"] > 1)
d = out["device"]
kernels = d["group_ms"] + d["mark_ms"] + d["emit_ms"]
out["kernels_ms"] = kernels
out["kernels_over_fills"] = kernels / fills_ms
out["expectation_held"] = dict(end_to_end=out["device_faster_than_host"], kernels_under_half_a_ms=bool(kernels < 0.5),
                               marking_longest=bool(d["mark_ms"] >= max(d["group_ms"], d["emit_ms"])), below_the_fills=bool(kernels < fills_ms))
cb.close(); ch.close()
print(json.dumps(out))
with open(os.path.join(ROOT, "profiles", "select_rate.json"), "w") as f:
    json.dump(out, f, indent=1)
    f.write("\n")
sys.exit(0 if agree and out["device_faster_than_host"] else 1)
