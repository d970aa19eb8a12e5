"""Device-side known-answer test of k_multi's in-lane gap scan in the order its loop of steps holds a lane's eight cells (round 7): register k =
cells k and k + 4, one packed chain over both halves (`scan_halves`), the scan over the slot's lanes (`multi_carry<16 / 32 / 64>`), one carry
across the halves (`apply_halves`).

The forms of `tests/test_gpu_lane_kat.py`, for the slots of 16, 32 and 64 lanes (columns of 128, 256 and 512 cells): expected values come from the
oracle's `simd_prefix_scan_i16` restatement, vector by vector, with the carry applied as the reference does (`scan_block.rs:1144-1150`), so the
zero-shift-in artefact of `avx2.rs:315-338` (`MultiConsts::w0`) has to come out the same.
"""
import numpy as np
import pytest

from tests.test_gpu_lane_kat import device_scan, expected_columns

pytestmark = pytest.mark.gpu

FORMS = {5: (128, "16 lanes x 8 cells (k, k + 4)"), 6: (256, "32 lanes x 8 cells (k, k + 4)"), 7: (512, "64 lanes x 8 cells (k, k + 4)")}   # form -> (cells per column, what)
PER_WAVE = 512


def whole_waves(x):
    pad = (-x.size) % PER_WAVE
    return np.concatenate([x, np.zeros(pad, np.int16)]) if pad else x


@pytest.mark.parametrize("form", sorted(FORMS))
def test_reference_prefix_scan_vectors(devlib, oracle, kats, form):
    """avx2.rs:476-486: the reference's two answers, as the first vector of a device column."""
    height, what = FORMS[form]
    seen = 0
    for k in kats["lane"]:
        if k["op"] != "prefix_scan":
            continue
        col = np.full(height, -30000, np.int16)
        col[:16] = k["input"]
        x = whole_waves(col)
        got = device_scan(devlib, form, x, k["gap"])
        assert list(got[:16]) == k["expect"], (what, k["name"], list(got[:16]))
        assert np.array_equal(got, expected_columns(oracle, x, height, k["gap"])), (what, k["name"])
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("form", sorted(FORMS))
def test_lane_scan_against_the_oracle(devlib, oracle, form):
    """The distributions and gaps of test_gpu_lane_kat.py: the whole int16 range, all negative, near both saturation bounds, around the MIN = 0
    sentinel, sparse columns; gap_extend -1 .. -128. 4096 vectors per distribution and gap."""
    height, what = FORMS[form]
    rng = np.random.default_rng(4321 + form)
    n_cells = 16 * 4096
    total = 0
    for g in (-1, -2, -3, -7, -16, -100, -128):
        for name, gen in (("uniform", lambda n: rng.integers(-32768, 32768, n)), ("negative", lambda n: rng.integers(-32768, 0, n)),
                          ("low", lambda n: rng.integers(-32768, -32000, n)), ("high", lambda n: rng.integers(32000, 32768, n)),
                          ("around the sentinel", lambda n: rng.integers(-40, 41, n)),
                          ("sparse", lambda n: np.where(rng.random(n) < 0.05, rng.integers(-32768, 32768, n), -32768))):
            x = gen(n_cells).astype(np.int16)
            got = device_scan(devlib, form, x, g)
            exp = expected_columns(oracle, x, height, g)
            bad = np.flatnonzero(got != exp)
            assert bad.size == 0, (what, g, name, int(bad[0]) % height, x[bad[0] - bad[0] % 16: bad[0] - bad[0] % 16 + 16], got[bad[0]], exp[bad[0]])
            total += n_cells // 16
    assert total >= 100000
