"""Anchor-chain batches without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, every argument
rejection is reported before the device is touched, and the splice kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from block_aligner_amd import scores as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_chain_batch_create", "ba_chain_batch_reload", "ba_chain_batch_run", "ba_chain_batch_results", "ba_chain_batch_cigars",
         "ba_chain_batch_times", "ba_chain_batch_destroy")
CALLER = r"""
#include "block_aligner_hip.h"
int use(const NucMatrix* m, const uint8_t* pool, const uint64_t* off, const uint32_t* len, const uint64_t* first, const uint32_t* anchor,
        const uint8_t* strand) {
    struct Gaps g = {-2, -1};
    struct SizeRange sz = {32, 256};
    BaChainBatch* b = ba_chain_batch_create(BA_KIND_NUC, m, g, sz, 50, BA_X_DROP | BA_TRACE, pool, off, len, off, len, first, anchor, anchor, len, strand, 1);
    float ms = 0.0f, e, gp, pk, sp;
    int32_t score; uint32_t qs, rs, qe, re, cl, st; int32_t ls, rsc; uint64_t cells; uint32_t runs[8];
    int rc = ba_chain_batch_reload(b, pool, off, len, off, len, first, anchor, anchor, len, NULL, 1);
    rc |= ba_chain_batch_run(b, &ms);
    rc |= ba_chain_batch_results(b, &score, &qs, &rs, &qe, &re, &ls, &rsc, &cells, &cl, &st);
    rc |= ba_chain_batch_cigars(b, runs, 8);
    rc |= ba_chain_batch_times(b, &e, &gp, &pk, &sp);
    rc |= ba_chain_batch_times(b, NULL, NULL, NULL, NULL);
    ba_chain_batch_destroy(b);
    return rc;
}
"""


def test_chain_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_chain_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
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


def _make(hip, matrix=None, mode=None, strand=None, **over):
    """Two chains over small DNA sequences: chain 0 has three anchors, chain 1 one."""
    a = dict(pool=np.frombuffer(b"ACGTACGTACGTTTGACCAGT" * 4, dtype=np.uint8),
             q_off=np.array([0, 10], np.uint64), q_len=np.array([40, 30], np.uint32),
             r_off=np.array([20, 5], np.uint64), r_len=np.array([30, 40], np.uint32),
             anchor_first=np.array([0, 3, 4], np.uint64),
             q_anchor=np.array([2, 10, 20, 10], np.uint32), r_anchor=np.array([1, 8, 14, 2], np.uint32), anchor_len=np.array([4, 5, 6, 15], np.uint32))
    a.update(over)
    return hip.ChainBatchAligner(matrix if matrix is not None else S.NucMatrix.new_simple(1, -1), (-2, -1), (32, 256), 20,
                                 hip.X_DROP | hip.TRACE if mode is None else mode, a["pool"], a["q_off"], a["q_len"], a["r_off"], a["r_len"],
                                 a["anchor_first"], a["q_anchor"], a["r_anchor"], a["anchor_len"], strand)


def _no_device(hip):
    try:
        return hip.device_count() < 1
    except Exception:
        return True


def test_a_valid_set_passes_every_check(hip):
    """The set the rejections below are cut from is itself accepted: without a device it gets as far as the device."""
    if not _no_device(hip):
        _make(hip).close()
        return
    with pytest.raises(RuntimeError, match="no usable HIP device"):
        _make(hip)


def test_rejects_missing_x_drop(hip):
    with pytest.raises(RuntimeError, match="chain batches need BA_X_DROP"):
        _make(hip, mode=hip.TRACE)


@pytest.mark.parametrize("flag", ["LOCAL_START", "FREE_QUERY_START_GAPS", "FREE_QUERY_END_GAPS"])
def test_rejects_special_modes(hip, flag):
    with pytest.raises(RuntimeError, match="LOCAL_START and FREE_QUERY_\\* are rejected"):
        _make(hip, mode=hip.X_DROP | getattr(hip, flag))


def test_rejects_a_chain_without_anchors(hip):
    with pytest.raises(RuntimeError, match="chain 1: a chain must hold at least one anchor"):
        _make(hip, anchor_first=np.array([0, 4, 4], np.uint64))


def test_rejects_empty_anchor(hip):
    with pytest.raises(RuntimeError, match="chain 0, anchor 1: anchor_len must be at least 1"):
        _make(hip, anchor_len=np.array([4, 0, 6, 15], np.uint32))


def test_rejects_overlapping_anchors_on_the_query(hip):
    with pytest.raises(RuntimeError, match="chain 0, anchor 1: the anchor overlaps or precedes anchor 0 on the query"):
        _make(hip, q_anchor=np.array([2, 5, 20, 10], np.uint32))   # anchor 0 ends at 6


def test_rejects_anchors_out_of_order_on_the_reference(hip):
    with pytest.raises(RuntimeError, match="chain 0, anchor 2: the anchor overlaps or precedes anchor 1 on the reference"):
        _make(hip, r_anchor=np.array([1, 8, 3, 2], np.uint32))


def test_rejects_anchor_past_the_end(hip):
    with pytest.raises(RuntimeError, match="chain 0, anchor 2: the anchor .* runs past the end"):
        _make(hip, anchor_len=np.array([4, 5, 17, 15], np.uint32))   # reference: 14 + 17 > 30
    with pytest.raises(RuntimeError, match="chain 1, anchor 0: the anchor .* runs past the end"):
        _make(hip, q_anchor=np.array([2, 10, 20, 16], np.uint32))    # query: 16 + 15 > 30


def test_rejects_anchor_first_not_from_zero(hip):
    with pytest.raises(RuntimeError, match="anchor_first must start at 0"):
        _make(hip, anchor_first=np.array([1, 3, 4], np.uint64))


def test_rejects_decreasing_anchor_first(hip):
    with pytest.raises(RuntimeError, match="chain 1: anchor_first must not decrease"):
        _make(hip, q_off=np.array([0, 10, 0], np.uint64), q_len=np.array([40, 30, 40], np.uint32), r_off=np.array([20, 5, 20], np.uint64),
              r_len=np.array([30, 40, 30], np.uint32), anchor_first=np.array([0, 3, 2, 4], np.uint64))


def test_rejects_bad_strand_value(hip):
    with pytest.raises(RuntimeError, match="chain 0: strand must be 0 or 1"):
        _make(hip, strand=np.array([2, 0], np.uint8))


def test_rejects_strand_on_amino_acids(hip):
    with pytest.raises(RuntimeError, match="chain 1: strand needs a NucMatrix"):
        _make(hip, matrix=S.static_matrix("BLOSUM62"), mode=hip.X_DROP, strand=np.array([0, 1], np.uint8),
              pool=np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY" * 4, dtype=np.uint8))


def test_rejects_mismatched_arrays(hip):
    with pytest.raises(ValueError, match="one entry per chain"):
        _make(hip, q_len=np.array([40], np.uint32))
    with pytest.raises(ValueError, match="one entry per chain and one more"):
        _make(hip, anchor_first=np.array([0, 4], np.uint64))
    with pytest.raises(ValueError, match="one entry per anchor"):
        _make(hip, q_anchor=np.array([2, 10, 20], np.uint32))
    with pytest.raises(ValueError, match="one entry per chain"):
        _make(hip, strand=np.array([0], np.uint8))


def test_null_batches_are_refused(hip):
    L = hip.lib()
    ms = ctypes.c_float()
    assert L.ba_chain_batch_run(None, ctypes.byref(ms)) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_results(None, *([None] * 10)) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_cigars(None, None, 0) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_times(None, None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_reload(None, *([None] * 10), 0) != 0 and "null batch" in hip.last_error()
    L.ba_chain_batch_destroy(None)
    one = np.zeros(2, np.uint64)
    assert not L.ba_chain_batch_create(1, None, hip.GapsC(-2, -1), hip.SizeRangeC(32, 128), 10, hip.X_DROP, *([one.ctypes.data] * 10), 1)
    assert "null argument" in hip.last_error()
    raw = S.NucMatrix.new_simple(1, -1).raw()
    assert not L.ba_chain_batch_create(1, raw.ctypes.data, hip.GapsC(-2, -1), hip.SizeRangeC(32, 128), 10, hip.X_DROP, None, *([one.ctypes.data] * 9), 1)
    assert "null argument" in hip.last_error()


def test_what_a_chain_batch_does_not_offer_says_so(hip):
    cb = object.__new__(hip.ChainBatchAligner)   # (no device: the class alone)
    cb._h = None
    for name in ("stats", "text", "text_list", "exact", "exact_cigars", "exact_paths", "accuracy"):
        with pytest.raises(RuntimeError, match="out of scope"):
            getattr(cb, name)()
    assert hip.ChainBatchAligner.RESULTS == hip.ExtendBatchAligner.RESULTS


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_chain_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_chain.hip"), "-o", str(tmp_path / "ba_chain.o")], capture_output=True, text=True)
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
    assert len(scratch) == 3 and set(scratch.values()) == {0}, scratch   # every kernel of the unit
    for k in ("k_chain_anchors", "k_chain_results", "k_chain_gather"):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0], (k, scratch)
    assert not [f for f in scratch if "k_pack_images" in f or "k_extend_" in f]   # (tests/test_extend_abi.py counts those by name)


def test_kernel_hash_lists_the_chain_sources():
    from tools import kernel_hash
    assert "ba_chain.hip" in kernel_hash.FILES and "ba_chain.h" in kernel_hash.FILES
