"""bench.py's argument handling (CPU): `--gpus N` without torch.distributed.run must not refuse to run (exit code 2) -- it takes the
one-process multi-GPU launcher (ba_multibatch_*), which then fails loudly here because no device is visible (there is no CPU fallback)."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], capture_output=True, text=True, env=env, timeout=600)


def test_gpus_n_without_a_launcher_takes_the_multibatch_path(hip):
    if hip.device_count() >= 2:
        pytest.skip("two devices are visible: the GPU tests run this path for real")
    r = run_bench("--gpus", "2", "--pairs", "8", "--len", "300", "--edits", "10", "--tail", "10", "--steps", "1", "--warmup", "0", "--gen-workers", "1")
    assert r.returncode != 2, r.stderr[-400:]
    assert "library's multi-GPU launcher" in r.stderr
    assert "HIP devices visible" in r.stderr and r.returncode != 0      # fails loudly, after the argument handling, for lack of devices
    assert "launch with torch.distributed.run" not in r.stderr


def test_world_size_mismatch_is_reported_not_fatal_for_one_gpu(hip):
    """--gpus 1 under no launcher is the plain form; the parser accepts every documented flag."""
    r = run_bench("--help")
    assert r.returncode == 0
    for flag in ("--gpus", "--steps", "--warmup", "--strong", "--multibatch", "--pairs"):
        assert flag in r.stdout


def test_dump_outputs_writes_a_seeded_bounded_sample(tmp_path, monkeypatch):
    """--dump-outputs (CPU, on made-up results): float64 files, the per-pair arrays whole or a seeded sample, the CIGAR runs of a seeded sample
    of pairs exactly as the caller received them, everything within the byte budget and the same from call to call."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    rng = np.random.default_rng(3)
    n = 5000
    cl = rng.integers(0, 300, n).astype(np.uint32)
    off = np.zeros(n + 1, np.uint64)
    np.cumsum(cl, out=off[1:])
    runs = rng.integers(0, 1 << 20, int(off[-1])).astype(np.uint32)
    res = dict(score=rng.integers(-500, 500, n).astype(np.int32), query_idx=rng.integers(0, 1 << 14, n).astype(np.uint32),
               reference_idx=rng.integers(0, 1 << 14, n).astype(np.uint32), cells=rng.integers(0, 1 << 40, n).astype(np.uint64),
               cigar_len=cl, status=np.zeros(n, np.uint32))
    for budget in (64 * 10**6, 200000):
        monkeypatch.setattr(bench, "DUMP_BYTES", budget)
        names = bench.dump_outputs(np, str(tmp_path / "a"), res, runs, off)
        assert bench.dump_outputs(np, str(tmp_path / "b"), res, runs, off) == names
        got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in names}
        assert all(v.dtype == np.float64 for v in got.values())
        assert all(np.array_equal(v, np.load(tmp_path / "b" / (k + ".npy"))) for k, v in got.items())
        assert sum(v.nbytes for v in got.values()) <= budget
        idx = got["pair_index"].astype(np.int64)
        assert len(idx) == (n if budget > 10**6 else len(idx)) and len(idx) > 0 and np.all(np.diff(idx) > 0)
        for f in ("score", "query_idx", "reference_idx", "cells", "status", "cigar_len"):
            assert np.array_equal(got[f], res[f][idx].astype(np.float64)), f
        pick, co = got["cigar_pairs"].astype(np.int64), got["cigar_offsets"].astype(np.int64)
        assert len(pick) == (1024 if budget > 10**6 else len(pick)) and len(pick) > 0 and co[-1] == len(got["cigar_runs"])
        for k, p in enumerate(pick):
            assert np.array_equal(got["cigar_runs"][co[k]: co[k + 1]], runs[int(off[p]): int(off[p + 1])].astype(np.float64)), p
    assert len(idx) < n and len(pick) < 1024      # (the small budget did cut both samples)


@pytest.mark.gpu
def test_dump_outputs_holds_what_the_timed_steps_computed(hip, oracle, tmp_path):
    """bench.py --dump-outputs on a small batch: --steps timed steps, `ms_per_step` in the line, and the dumped scores, end positions, cells and
    CIGAR runs are the oracle's for the same seeded input."""
    import json
    import numpy as np
    from block_aligner_amd import workloads as W
    from block_aligner_amd.shard import shard_seed
    d = tmp_path / "dump"
    r = run_bench("--gpus", "1", "--pairs", "600", "--len", "1000", "--edits", "100", "--tail", "50", "--steps", "2", "--warmup", "1",
                  "--gen-workers", "1", "--no-cpu-baseline", "--no-secondary", "--no-e2e", "--dump-outputs", str(d))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert np.array_equal(got["pair_index"], np.arange(600)) and not got["status"].any()
    w = W.config3(600, 1000, 100, 50, seed=shard_seed(1234, 0), trace=True, size=(hip.percent_len(1000, 0.01), hip.percent_len(1000, 0.1)))
    p = w.pairs
    ref = oracle.batch_align(w.matrix, p.pool, p.q_off, p.q_len, p.r_off, p.r_len, w.gaps, w.size, w.x_drop, w.mode, cigar_eq=True)
    assert np.array_equal(got["score"], ref["scores"]) and np.array_equal(got["query_idx"], ref["query_idx"])
    assert np.array_equal(got["reference_idx"], ref["reference_idx"]) and int(got["cells"].sum()) == ref["cells"]
    assert np.array_equal(got["cigar_len"], ref["cig_len"])
    co = got["cigar_offsets"].astype(np.int64)
    for k, q in enumerate(got["cigar_pairs"].astype(np.int64)):
        o = int(ref["cig_off"][q])
        assert np.array_equal(got["cigar_runs"][co[k]: co[k + 1]], ref["cig_ops"][o: o + int(ref["cig_len"][q])]), q
