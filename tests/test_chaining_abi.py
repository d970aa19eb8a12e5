"""Anchor chaining without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, struct BaChainingParams is
36 bytes, every argument rejection is reported before the device is touched, and the kernels compile for gfx950 without scratch."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import chaining_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_chaining_create", "ba_chaining_reload", "ba_chaining_run", "ba_chaining_counts", "ba_chaining_results", "ba_chaining_dp",
         "ba_chaining_times", "ba_chaining_destroy")
CALLER = r"""
#include "block_aligner_hip.h"
typedef char params_are_36_bytes[sizeof(struct BaChainingParams) == 36 ? 1 : -1];
int use(const uint64_t* first, const uint32_t* anchor, const uint32_t* len) {
    struct BaChainingParams p = {4, 1, 0, 64, 500, 100, 3, 20, 1};
    BaChaining* b = ba_chaining_create(&p, first, anchor, anchor, len, 1);
    float ms = 0.0f, f, pk, g;
    uint64_t nc, na, out_first[4]; uint32_t per[1], prob[3], rank[3], q[8], r[8], l[8], src[8]; int32_t score[3], dpf[8], pred[8];
    int rc = ba_chaining_reload(b, first, anchor, anchor, len, 1);
    rc |= ba_chaining_run(b, &ms);
    rc |= ba_chaining_counts(b, &nc, &na, per);
    rc |= ba_chaining_results(b, prob, rank, score, out_first, q, r, l, src);
    rc |= ba_chaining_dp(b, dpf, pred);
    rc |= ba_chaining_times(b, &f, &pk, &g);
    rc |= ba_chaining_times(b, NULL, NULL, NULL);
    ba_chaining_destroy(b);
    return rc;
}
"""
GOOD = R.Params(4, 1, 1, 64, 400, 60, 4, 24, 2)


def test_chaining_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_chaining_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)   # (holds the size of the struct as a compile-time check)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_params_are_nine_4_byte_fields(hip):
    assert ctypes.sizeof(hip.ChainingParamsC) == 36
    assert [f[0] for f in hip.ChainingParamsC._fields_] == list(R.Params._fields)
    assert all(ctypes.sizeof(f[1]) == 4 for f in hip.ChainingParamsC._fields_)


def _make(hip, P=GOOD, **over):
    """Two problems: the known answer's eight anchors, and three more."""
    ps = R.ProblemSet([(R.KNOWN_Q, R.KNOWN_R, R.KNOWN_L), ([5, 9, 30], [7, 11, 30], [8, 8, 10])])
    a = dict(anchor_first=ps.anchor_first, q_anchor=ps.q_anchor, r_anchor=ps.r_anchor, anchor_len=ps.anchor_len)
    a.update(over)
    return hip.AnchorChainer(*P, a["anchor_first"], a["q_anchor"], a["r_anchor"], a["anchor_len"])


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


@pytest.mark.parametrize("change, message", [
    (dict(match_w=0), "match_w must be at least 1"),
    (dict(drift_cost=-1), "drift_cost and skip_cost must not be negative"),
    (dict(skip_cost=-2), "drift_cost and skip_cost must not be negative"),
    (dict(lookback=0), "lookback must be between 1 and 1024"),
    (dict(lookback=1025), "lookback must be between 1 and 1024"),
    (dict(max_dist=0), "max_dist must be at least 1"),
    (dict(max_chains=0), "max_chains must be between 1 and 64"),
    (dict(max_chains=65), "max_chains must be between 1 and 64"),
    (dict(min_anchors=0), "min_anchors must be at least 1"),
    (dict(drift_cost=1 << 20, bandwidth=1 << 10), r"drift_cost \* bandwidth \+ skip_cost \* max_dist must stay below 2\^30"),
    (dict(skip_cost=1 << 18, max_dist=1 << 12), r"drift_cost \* bandwidth \+ skip_cost \* max_dist must stay below 2\^30"),
])
def test_rejects_parameters_out_of_range(hip, change, message):
    with pytest.raises(RuntimeError, match=message):
        _make(hip, GOOD._replace(**change))


def test_accepts_the_largest_parameters(hip):
    """2^30 - 1 in costs is allowed, as are a lookback of 1024 and 64 chains."""
    P = GOOD._replace(drift_cost=(1 << 30) - 1, bandwidth=1, skip_cost=0, lookback=1024, max_chains=64)
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            _make(hip, P)
    else:
        _make(hip, P).close()


def test_rejects_empty_anchor(hip):
    L = np.array(R.KNOWN_L + [8, 0, 10], np.uint32)
    with pytest.raises(RuntimeError, match="problem 1, anchor 1: anchor_len must be at least 1"):
        _make(hip, anchor_len=L)


def test_rejects_unsorted_anchors(hip):
    q = np.array(R.KNOWN_Q + [5, 9, 30], np.uint32)
    r = np.array(R.KNOWN_R + [7, 30, 11], np.uint32)
    with pytest.raises(RuntimeError, match=r"problem 1, anchor 2: the anchors must be sorted by \(reference end, query end\)"):
        _make(hip, q_anchor=q, r_anchor=r)
    q = np.array(R.KNOWN_Q + [5, 4, 30], np.uint32)   # equal reference ends: the query end decides
    r = np.array(R.KNOWN_R + [7, 7, 30], np.uint32)
    with pytest.raises(RuntimeError, match=r"problem 1, anchor 1: the anchors must be sorted"):
        _make(hip, q_anchor=q, r_anchor=r, anchor_len=np.array(R.KNOWN_L + [8, 8, 10], np.uint32))


def test_equal_keys_are_sorted(hip):
    q = np.array(R.KNOWN_Q + [5, 5, 30], np.uint32)
    r = np.array(R.KNOWN_R + [7, 7, 30], np.uint32)
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            _make(hip, q_anchor=q, r_anchor=r)
    else:
        _make(hip, q_anchor=q, r_anchor=r).close()


def test_rejects_ends_from_2_31(hip):
    q = np.array(R.KNOWN_Q + [5, 9, (1 << 31) - 10], np.uint32)
    with pytest.raises(RuntimeError, match=r"problem 1, anchor 2: the anchor ends at query 2147483648, reference 40: both must stay below 2\^31"):
        _make(hip, q_anchor=q)
    r = np.array(R.KNOWN_R + [7, 11, (1 << 32) - 5], np.uint32)   # (the end is computed in 64 bits)
    with pytest.raises(RuntimeError, match=r"problem 1, anchor 2: the anchor ends at query 40, reference 4294967301"):
        _make(hip, r_anchor=r)


def test_rejects_a_score_that_leaves_int32(hip):
    L = np.array(R.KNOWN_L + [8, 8, 1 << 20], np.uint32)
    q = np.array(R.KNOWN_Q + [5, 9, 30], np.uint32)
    with pytest.raises(RuntimeError, match=r"problem 1: match_w \* the sum of anchor_len must stay below 2\^31"):
        _make(hip, GOOD._replace(match_w=2048), q_anchor=q, anchor_len=L)


def test_rejects_anchor_first_not_from_zero(hip):
    with pytest.raises(RuntimeError, match="anchor_first must start at 0"):
        _raw_create(hip, np.array([1, 8, 11], np.uint64))


def test_rejects_decreasing_anchor_first(hip):
    with pytest.raises(RuntimeError, match="problem 1: anchor_first must not decrease"):
        _raw_create(hip, np.array([0, 8, 5, 11], np.uint64), n=3)


def _raw_create(hip, first, n=2):
    """(The binding sizes the arrays by anchor_first[-1] itself: the C call is made directly.)"""
    P = hip.ChainingParamsC(*GOOD)
    x = np.ones(16, np.uint32)
    h = hip.lib().ba_chaining_create(ctypes.byref(P), first.ctypes.data, x.ctypes.data, x.ctypes.data, x.ctypes.data, n)
    if not h:
        raise RuntimeError(hip.last_error())
    hip.lib().ba_chaining_destroy(h)


def test_rejects_mismatched_arrays(hip):
    with pytest.raises(ValueError, match="one entry per anchor"):
        _make(hip, q_anchor=np.array([2, 10, 20], np.uint32))
    with pytest.raises(ValueError, match="one entry per problem and one more"):
        _make(hip, anchor_first=np.zeros(0, np.uint64))


def test_null_batches_and_null_arguments_are_refused(hip):
    L = hip.lib()
    ms = ctypes.c_float()
    assert L.ba_chaining_run(None, ctypes.byref(ms)) != 0 and "null batch" in hip.last_error()
    assert L.ba_chaining_counts(None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_chaining_results(None, *([None] * 8)) != 0 and "null batch" in hip.last_error()
    assert L.ba_chaining_dp(None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_chaining_times(None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_chaining_reload(None, *([None] * 4), 0) != 0 and "null batch" in hip.last_error()
    L.ba_chaining_destroy(None)
    one = np.zeros(2, np.uint64)
    P = hip.ChainingParamsC(*GOOD)
    assert not L.ba_chaining_create(None, *([one.ctypes.data] * 4), 1) and "null argument" in hip.last_error()
    for k in range(4):
        args = [one.ctypes.data] * 4
        args[k] = None
        assert not L.ba_chaining_create(ctypes.byref(P), *args, 1) and "null argument" in hip.last_error(), k


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_chaining_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_chaining.hip"), "-o", str(tmp_path / "ba_chaining.o")], capture_output=True, text=True)
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
    for k in ("k_chaining_fill", "k_chaining_pick", "k_chaining_gather"):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0], (k, scratch)


def test_kernel_hash_lists_the_chaining_sources():
    from tools import kernel_hash
    assert "ba_chaining.hip" in kernel_hash.FILES and "ba_chaining.h" in kernel_hash.FILES
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    assert re.search(r"^XOBJS := .*\$\(OBJ\)/ba_chaining\.o", mk, flags=re.M) and re.search(r"^HDRS := .*\bba_chaining\.h\b", mk, flags=re.M)
