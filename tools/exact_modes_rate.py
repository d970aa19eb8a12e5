#!/usr/bin/env python3
"""Rate of the exact full-matrix scores in a batch's own mode (ba_batch_exact with BA_EXACT_OWN_MODE, DESIGN.md "Exact scores in the
batch's own mode") beside the plain form at the same shapes:
  dna      2000 DNA pairs of about 1 kbp, NucMatrix, BA_EXACT_GLOBAL: plain, LOCAL_START, FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS
  protein  2000 protein pairs of about 300, BLOSUM62: the plain form over sequence pairs, the profile form over PSSMs of the references
Per form `--runs` timed calls after one that allocates (HIP events, ba_batch_exact_ms): every time, the median, cells per second.
--parent-tree names a built checkout of the parent commit: the plain forms are measured on its package and library too, and its largest
minus smallest time is the run-to-run spread the plain form of this tree is held against.
Every form runs in a child process of its own under `timeout`, one after the other; the first one that fails ends the script.
Writes profiles/exact_modes_rate.json (or --out); no such record has been taken yet.
usage: exact_modes_rate.py [--out FILE] [--runs N] [--pairs N] [--parent-tree DIR] [--parent-commit ID] [--commit ID]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP_SECONDS = 120
DNA_FORMS = ("plain", "local_start", "free_query_start_gaps", "free_query_end_gaps")


def step(name: str, n: int, runs: int, tree: str) -> dict:
    import numpy as np
    sys.path.insert(0, tree or ROOT)
    from block_aligner_amd import hip as H, scores as S, synth
    own = name not in ("dna:plain", "protein:plain")
    if name.startswith("dna:"):
        pairs = synth.make_pairs(n, 1000, 100, 50, synth.DNA, seed=901)
        mode = {"plain": 0, "local_start": H.LOCAL_START, "free_query_start_gaps": H.FREE_QUERY_START_GAPS, "free_query_end_gaps": H.FREE_QUERY_END_GAPS}[name[4:]]
        # (FREE_QUERY_END_GAPS: the minimum block must exceed every query; nothing is run, the block range sizes the padding only)
        b = H.BatchAligner(S.NucMatrix.new_simple(2, -3), (-5, -1), (2048, 2048), 0, mode, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    else:
        pairs = synth.make_pairs(n, 300, 30, 15, synth.AMINO, seed=902)
        if name == "protein:plain":
            b = H.BatchAligner(S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 0, 0, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
        else:
            table = np.asarray(S.static_matrix("BLOSUM62").scores, np.int8).reshape(27, 32)
            profiles = []
            for p in range(len(pairs)):
                cons = np.frombuffer(pairs.reference(p), np.uint8).astype(np.int64) - 65
                pr = S.AAProfile(len(cons), 256, -1)
                pr.pos_aa[1: len(cons) + 1] = table[cons]
                pr.set_all_gap_open_C(-10); pr.set_all_gap_close_C(0); pr.set_all_gap_open_R(-10)
                profiles.append(pr)
            b = H.ProfileBatchAligner(profiles, (32, 256), 0, 0, pairs.pool, pairs.q_off, pairs.q_len)
    what = H.EXACT_GLOBAL | (H.EXACT_OWN_MODE if own else 0)      # (the plain forms must run on the parent's package, which has no flag)
    b.exact(what)                      # (allocates the row buffers)
    times = []
    for _ in range(runs):
        b.exact(what)
        ms, cells = b.exact_ms()
        times.append(ms)
    b.close()
    med = float(np.median(times))
    return dict(form=name, pairs=len(pairs), cells=cells, ms=[float(t) for t in times], ms_median=med, ms_min=float(min(times)), ms_max=float(max(times)),
                gcups=cells / med / 1e6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exact_modes_rate.json"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=2000)
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--parent-commit", default="")
    ap.add_argument("--commit", default="")
    ap.add_argument("--step", help=argparse.SUPPRESS)
    ap.add_argument("--tree", default="", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        print("RESULT " + json.dumps(step(a.step, a.pairs, a.runs, a.tree)))
        return 0
    sys.path.insert(0, ROOT)
    from tools.kernel_hash import kernel_hash
    out = dict(kernel_hash=kernel_hash(), commit=a.commit, parent_commit=a.parent_commit, repeats=a.runs, pairs=a.pairs, parent={}, forms={})
    steps = [("parent", f, os.path.abspath(a.parent_tree)) for f in ("dna:plain", "protein:plain") if a.parent_tree]
    steps += [("forms", f"dna:{f}", "") for f in DNA_FORMS] + [("forms", "protein:plain", ""), ("forms", "protein:profile", "")]
    for where, name, tree in steps:
        r = subprocess.run(["timeout", "-k", "10", str(STEP_SECONDS), sys.executable, os.path.abspath(__file__), "--step", name, "--pairs", str(a.pairs),
                            "--runs", str(a.runs), "--tree", tree], capture_output=True, text=True)
        if r.returncode != 0:   # nothing more is started on the device after a failure
            sys.stderr.write(r.stdout + r.stderr)
            print(f"exact_modes_rate: step {name} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        out[where][name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(where, json.dumps(out[where][name]), flush=True)
    f = out["forms"]
    out["ratio_to_plain"] = {k[4:]: f[k]["ms_median"] / f["dna:plain"]["ms_median"] for k in f if k.startswith("dna:") and k != "dna:plain"}
    out["profile_cells_per_second"] = f["protein:profile"]["cells"] / f["protein:profile"]["ms_median"] * 1e3
    if a.parent_tree:
        out["plain_against_parent"] = {
            k: dict(parent_spread_ms=out["parent"][k]["ms_max"] - out["parent"][k]["ms_min"], parent_ms_median=out["parent"][k]["ms_median"],
                    ms_median=f[k]["ms_median"], slower_by_ms=f[k]["ms_median"] - out["parent"][k]["ms_median"],
                    within_parent_spread=f[k]["ms_median"] - out["parent"][k]["ms_median"] <= out["parent"][k]["ms_max"] - out["parent"][k]["ms_min"])
            for k in ("dna:plain", "protein:plain")}
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
