#!/usr/bin/env python3
"""Rate of the traced own-mode exact kernels (ba_batch_exact_paths: sweep with trace, walk, offsets, gather) against the
untraced ones (ba_batch_exact with BA_EXACT_OWN_MODE) on the same pairs, samples of
  local    1 kbp DNA reads in a LOCAL_START batch, EXTEND over the whole matrix
  profile  protein queries against position-specific profiles of their references, GLOBAL
Per configuration: HIP-event time of `runs` calls of each form, interleaved (the median, the minimum and the maximum), cells, GCUPS, and
the ratio traced / untraced of the median times with the spread of the per-round ratios.
Every configuration runs in a child process of its own under `timeout`, one after the other; the first one that fails ends the script.
Writes profiles/exact_modes_trace_rate.json (or --out) with the kernel hash of the tree.
usage: exact_modes_trace_rate.py [--out FILE] [--runs N] [--local PAIRS] [--profile PAIRS]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEP_SECONDS = 240


def step(name: str, n: int, runs: int) -> dict:
    import numpy as np
    from block_aligner_amd import hip as H, scores as S, synth, workloads as W
    if name == "local":
        w = W.config2(n, workers=8)
        p = w.pairs
        b = H.BatchAligner(w.matrix, w.gaps, w.size, 0, H.LOCAL_START, p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
        what, label = H.EXACT_EXTEND, w.name + " LOCAL_START"
    else:
        p = synth.make_pairs(n, 400, 40, 40, synth.AMINO, seed=77)
        profiles = [S.AAProfile.from_bytes(p.reference(k), 512, 2, -1, -10, -1, -9, -1) for k in range(len(p))]
        b = H.ProfileBatchAligner(profiles, (32, 512), 0, 0, p.pool, p.q_off, p.q_len)
        what, label = H.EXACT_GLOBAL, "protein queries against profiles"
    one = np.zeros(1, np.uint32)
    b.exact(what, own_mode=True)             # (both forms allocate their buffers)
    rec, runs_, off = b.exact_paths(what)
    plain, traced = [], []
    for _ in range(runs):
        b.exact(what, own_mode=True)
        ms, cells = b.exact_ms()
        plain.append(ms)
        b.exact_paths(what, which=one)         # (another request: the next one computes again)
        b.exact_paths(what)
        ms, tcells = b.exact_paths_ms()
        traced.append(ms)
    b.close()
    assert tcells == cells
    ratios = [t / u for t, u in zip(traced, plain)]
    pm, tm = float(np.median(plain)), float(np.median(traced))
    return dict(workload=label, pairs=len(p), what="EXTEND" if what == H.EXACT_EXTEND else "GLOBAL", cells=cells, runs_total=int(off[-1]),
                untraced_ms=pm, untraced_ms_min=float(min(plain)), untraced_ms_max=float(max(plain)), untraced_gcups=cells / pm / 1e6,
                traced_ms=tm, traced_ms_min=float(min(traced)), traced_ms_max=float(max(traced)), traced_gcups=cells / tm / 1e6,
                ratio=tm / pm, ratio_min=float(min(ratios)), ratio_max=float(max(ratios)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_modes_trace_rate.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--local", type=int, default=20000)
    ap.add_argument("--profile", type=int, default=4096)
    ap.add_argument("--step", help=argparse.SUPPRESS)
    ap.add_argument("--pairs", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.pairs, a.runs)))
        return 0
    from tools.kernel_hash import kernel_hash
    out = dict(kernel_hash=kernel_hash(), runs=a.runs, configs={})
    for name, n in (("local", a.local), ("profile", a.profile)):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name, "--pairs", str(n),
                            "--runs", str(a.runs)], capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(r.stdout + r.stderr)
            print(f"exact_modes_trace_rate: step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        out["configs"][name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, json.dumps(out["configs"][name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
