#!/usr/bin/env python3
"""Rate of the exact full-matrix scores (ba_batch_exact, DESIGN.md "Exact scores") and the first accuracy record of the block heuristic,
on samples of the project's standard configurations at their standard block ranges:
  c3  10 kbp DNA reads, block 128..1024, X-drop 100 (the headline configuration; a sample of its pairs)
  c2  1 kbp DNA reads, block 32..256, X-drop 100
  c4  protein pairs (lognormal lengths), BLOSUM62, global, block 32..256
Per configuration: the heuristic fill (its kernel time, the cells it computed), the exact call (HIP-event time, cells, GCUPS; the median of
`runs` calls) and the accuracy summary of the fill's results against the exact records.
Every configuration runs in a child process of its own under `timeout`, one after the other; the first one that fails ends the script.
Writes profiles/exact_rate.json (or --out) with the kernel hash of the tree.
usage: exact_rate.py [--out FILE] [--runs N] [--c3 PAIRS] [--c2 PAIRS] [--c4 PAIRS]"""
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
    from block_aligner_amd import hip as H, workloads as W
    w = {"c3": lambda: W.config3(n, workers=8, trace=False, size=(128, 1024)), "c2": lambda: W.config2(n, workers=8), "c4": lambda: W.config4(n)}[name]()
    p = w.pairs
    mode = (H.X_DROP if "x_drop" in w.mode else 0)
    b = H.BatchAligner(w.matrix, w.gaps, w.size, w.x_drop, mode, p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
    b.run()
    fill_ms = float(np.median([b.run() for _ in range(runs)]))
    res = b.results()
    b.exact(x_drop=-1)                     # (allocates the row buffers)
    times = []
    for _ in range(runs):
        b.exact(x_drop=-1)
        ms, cells = b.exact_ms()
        times.append(ms)
    ms = float(np.median(times))
    acc = b.accuracy()
    info = b.info()
    b.close()
    fill_cells = int(res["cells"].sum())
    return dict(workload=w.name, pairs=len(p), block=list(w.size), x_drop=w.x_drop if mode else None, what="EXTEND" if mode else "GLOBAL",
                exact_cells=cells, exact_ms=ms, exact_ms_min=float(min(times)), exact_ms_max=float(max(times)), exact_gcups=cells / ms / 1e6,
                fill_kernel=info["kernel"], fill_ms=fill_ms, fill_cells=fill_cells, fill_gcups=fill_cells / fill_ms / 1e6,
                fill_full_matrix_gcups=w.full_matrix_cells() / fill_ms / 1e6, accuracy=acc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_rate.json"))
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--c3", type=int, default=4096)
    ap.add_argument("--c2", type=int, default=20000)
    ap.add_argument("--c4", type=int, default=20000)
    ap.add_argument("--step", help=argparse.SUPPRESS)
    ap.add_argument("--pairs", type=int, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.pairs, a.runs)))
        return 0
    from tools.kernel_hash import kernel_hash
    out = dict(kernel_hash=kernel_hash(), runs=a.runs, configs={})
    for name, n in (("c3", a.c3), ("c2", a.c2), ("c4", a.c4)):
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name, "--pairs", str(n),
                            "--runs", str(a.runs)], capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(r.stdout + r.stderr)
            print(f"exact_rate: step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        out["configs"][name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, json.dumps(out["configs"][name]), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
