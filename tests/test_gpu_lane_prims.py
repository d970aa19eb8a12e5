"""Device-side known answers of the single helpers the alignment kernels are built from, and of the sort and the search the seeding units share.

`ba_dev_lane_prim` (development library, `k_prim_kat` in ba_kernels.hip) runs ONE helper of ba_device.hpp / ba_quad.hpp / ba_multi.hpp / ba_small.hpp
(and `ffbl_u32` of ba_driver.hpp) per launch on caller-supplied operands: the DPP shifts and broadcasts, the swizzle / bpermute broadcasts, the adds and
maxima with a fused DPP control, the packed 16-bit arithmetic with its op_sel / clamp / SDWA modifiers, the v_perm shuffles, v_bfi, v_cndmask with a scalar
mask, the v_writelane parking. The kernel forms every operand as `x ^ kl` (kl: the low word of the wave-uniform k), so that a cross-lane helper reads a
register a VALU instruction has just written, as in the loops of steps; this file sends `a ^ kl` for the operands `a` it means. Expected values: the NumPy
models of tests/lane_prims_ref.py, exactly (everything is integer). The inputs are that module's: tests/test_lane_prims_ref.py shows without a GPU that
they tell every helper from the mistakes it could be confused with.

`ba_dev_sort_keys` (`k_sort_kat`) sorts uint64 keys in LDS with `ba::seed::sort_network<THREADS>` and looks every input key up with
`ba::seed::lower_bound`, against `np.sort` and `np.searchsorted(side="left")`.
"""
import ctypes as C

import numpy as np
import pytest

from tests import lane_prims_ref as R

pytestmark = pytest.mark.gpu


def device_prim(hip, o, a, k):
    """the helper of op `o` on operands a [waves, 64, 4] (int32 values) and the wave-uniform k -> [waves, 64, n_out]"""
    x = np.ascontiguousarray(R.i32(a ^ (k & 0xffffffff)).astype(np.int32))
    out = np.full(x.shape, 0x5eed, np.int32)
    f = hip.lib().ba_dev_lane_prim
    f.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    f.restype = C.c_int
    assert f(o.num, x.ctypes.data, x.shape[0] * 64, k, out.ctypes.data) == 0, hip.last_error()
    assert not out[..., o.n_out:].any(), (o.name, "words the op does not name are 0")
    return out[..., :o.n_out].astype(np.int64)


def device_sort(hip, threads, keys):
    n = len(keys)
    buf = np.concatenate([np.asarray(keys, np.uint64), np.full(n, 0xdead, np.uint64)])
    f = hip.lib().ba_dev_sort_keys
    f.argtypes = [C.c_int, C.c_void_p, C.c_uint32]
    f.restype = C.c_int
    assert f(threads, buf.ctypes.data, n) == 0, hip.last_error()
    return buf[:n], buf[n:]


@pytest.mark.parametrize("name", list(R.OPS))
def test_helper_against_its_model(devlib, name):
    o = R.OPS[name]
    for a, k in R.cases_of(o):
        got = device_prim(devlib, o, a, k)
        exp = R.model(o, a, k)
        bad = np.argwhere(got != exp)
        if bad.size:
            w, l, i = (int(v) for v in bad[0])
            lanes = slice(0, 64) if o.kind == "lane" else slice(l, l + 1)
            assert False, (f"{name} (op {o.num}), k = {k:#018x}: wave {w} lane {l} word {i}: device {int(got[w, l, i])}, model {int(exp[w, l, i])}; "
                           f"operands of {'the wave' if o.kind == 'lane' else 'the lane'}: {a[w, lanes].tolist()}")


def test_bad_arguments_are_refused(devlib):
    f = devlib.lib().ba_dev_lane_prim
    f.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    f.restype = C.c_int
    x = np.zeros((64, 4), np.int32)
    out = np.zeros_like(x)
    assert f(R.N_OPS, x.ctypes.data, 64, 0, out.ctypes.data) != 0 and "ba_dev_lane_prim" in devlib.last_error()
    assert f(-1, x.ctypes.data, 64, 0, out.ctypes.data) != 0
    assert f(0, None, 64, 0, out.ctypes.data) != 0 and f(0, x.ctypes.data, 64, 0, None) != 0
    assert f(0, x.ctypes.data, 0, 0, out.ctypes.data) != 0 and f(0, x.ctypes.data, 63, 0, out.ctypes.data) != 0
    g = devlib.lib().ba_dev_sort_keys
    g.argtypes = [C.c_int, C.c_void_p, C.c_uint32]
    g.restype = C.c_int
    k = np.zeros(4, np.uint64)
    assert g(128, k.ctypes.data, 2) != 0 and "ba_dev_sort_keys" in devlib.last_error()
    assert g(64, None, 2) != 0
    assert g(64, k.ctypes.data, R.SORT_THREADS[64] + 1) != 0 and g(1024, k.ctypes.data, R.SORT_THREADS[1024] + 1) != 0


@pytest.mark.parametrize("family", R.KEY_FAMILIES)
@pytest.mark.parametrize("threads", sorted(R.SORT_THREADS))
def test_sort_network_and_lower_bound(devlib, threads, family):
    """every size of the list and the largest counts the kernels of this THREADS sort in LDS (one below the bound, and the bound)"""
    for n in R.sort_sizes(threads):
        keys = R.sort_keys(family, n)
        got, lb = device_sort(devlib, threads, keys)
        exp, exp_lb = R.sort_expected(keys)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, (f"sort_network<{threads}>, {family}, n = {n}: entry {int(bad[0])}: device {int(got[bad[0]]):#x}, expected {int(exp[bad[0]]):#x}")
        bad = np.flatnonzero(lb != exp_lb)
        assert bad.size == 0, (f"lower_bound after sort_network<{threads}>, {family}, n = {n}: key {int(bad[0])} = {int(keys[bad[0]]):#x}: "
                               f"device {int(lb[bad[0]])}, expected {int(exp_lb[bad[0]])}")
