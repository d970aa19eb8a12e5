"""Seed-and-extend batches without a GPU: the C calls are exported and declared, every argument rejection is reported before the
device is touched, and the new kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from block_aligner_amd import scores as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_extend_batch_create", "ba_extend_batch_reload", "ba_extend_batch_run", "ba_extend_batch_results", "ba_extend_batch_cigars",
         "ba_extend_batch_destroy")
CALLER = r"""
#include "block_aligner_hip.h"
int use(const NucMatrix* m, const uint8_t* pool, const uint64_t* off, const uint32_t* len, const uint32_t* seed, const uint8_t* strand) {
    struct Gaps g = {-2, -1};
    struct SizeRange sz = {32, 256};
    BaExtendBatch* b = ba_extend_batch_create(BA_KIND_NUC, m, g, sz, 50, BA_X_DROP | BA_TRACE, pool, off, len, off, len, seed, seed, len, strand, 1);
    float ms = 0.0f;
    int32_t score; uint32_t qs, rs, qe, re, cl, st; int32_t ls, rsc; uint64_t cells; uint32_t runs[8];
    int rc = ba_extend_batch_reload(b, pool, off, len, off, len, seed, seed, len, NULL, 1);
    rc |= ba_extend_batch_run(b, &ms);
    rc |= ba_extend_batch_results(b, &score, &qs, &rs, &qe, &re, &ls, &rsc, &cells, &cl, &st);
    rc |= ba_extend_batch_cigars(b, runs, 8);
    rc |= ba_extend_batch_times(b, &ms, NULL, NULL);
    ba_extend_batch_destroy(b);
    return rc;
}
"""


def test_extend_symbols_are_exported(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert not [n for n in CALLS if not hasattr(lib, n)]


def test_extend_calls_are_declared(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _dna_set():
    pool = np.frombuffer(b"ACGTACGTACGTTTGACCAGT" * 4, dtype=np.uint8)
    n = 2
    q_off = np.array([0, 10], np.uint64); q_len = np.array([40, 30], np.uint32)
    r_off = np.array([20, 5], np.uint64); r_len = np.array([30, 40], np.uint32)
    q_seed = np.array([5, 10], np.uint32); r_seed = np.array([8, 2], np.uint32); seed_len = np.array([12, 15], np.uint32)
    return n, pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len


def _make(hip, matrix=None, mode=None, q_seed=None, seed_len=None, strand=None):
    n, pool, q_off, q_len, r_off, r_len, qs, rs, sl = _dna_set()
    return hip.ExtendBatchAligner(matrix if matrix is not None else S.NucMatrix.new_simple(1, -1), (-2, -1), (32, 256), 20,
                                  hip.X_DROP | hip.TRACE if mode is None else mode, pool, q_off, q_len, r_off, r_len,
                                  qs if q_seed is None else q_seed, rs, sl if seed_len is None else seed_len, strand)


def test_rejects_missing_x_drop(hip):
    with pytest.raises(RuntimeError, match="need BA_X_DROP"):
        _make(hip, mode=hip.TRACE)


@pytest.mark.parametrize("flag", ["LOCAL_START", "FREE_QUERY_START_GAPS", "FREE_QUERY_END_GAPS"])
def test_rejects_special_modes(hip, flag):
    with pytest.raises(RuntimeError, match="LOCAL_START and FREE_QUERY_\\* are rejected"):
        _make(hip, mode=hip.X_DROP | getattr(hip, flag))


def test_rejects_seed_past_the_end(hip):
    with pytest.raises(RuntimeError, match="seed 1: the seed .* runs past the end"):
        _make(hip, q_seed=np.array([5, 16], np.uint32))   # 16 + 15 > 30


def test_rejects_empty_seed(hip):
    with pytest.raises(RuntimeError, match="seed 0: seed_len must be at least 1"):
        _make(hip, seed_len=np.array([0, 15], np.uint32))


def test_rejects_strand_on_amino_acids(hip):
    pool = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY" * 4, dtype=np.uint8)
    with pytest.raises(RuntimeError, match="seed 1: strand needs a NucMatrix"):
        hip.ExtendBatchAligner(S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, hip.X_DROP, pool, [0, 10], [40, 30], [20, 5], [30, 40],
                               [5, 10], [8, 2], [12, 15], strand=[0, 1])


def test_rejects_bad_strand_value(hip):
    with pytest.raises(RuntimeError, match="seed 0: strand must be 0 or 1"):
        _make(hip, strand=np.array([2, 0], np.uint8))


def test_rejects_mismatched_arrays(hip):
    with pytest.raises(ValueError, match="one entry per seed"):
        _make(hip, q_seed=np.array([5], np.uint32))


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_extend_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_extend.hip"), "-o", str(tmp_path / "ba_extend.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scratch = {}
    name = None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    for k in ("k_pack_images", "k_extend_results", "k_extend_offsets", "k_extend_gather"):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0], (k, scratch)
