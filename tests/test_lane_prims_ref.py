"""The NumPy models of the device helpers (tests/lane_prims_ref.py), without a GPU: known answers written by hand for every cross-lane op, and the
condition on the GPU test's inputs -- on them every model differs from each mistake its helper could be confused with (another slot width, the other
direction, another value at the edge lane, first for last, low for high half, signed for unsigned, saturating for wrapping, split for join ...).
A variant put into a model in place of the model makes the second test fail: the inputs tell the two apart."""
import numpy as np
import pytest

from tests import lane_prims_ref as R

L = list(range(64))
KH = R.KH


def ramp(name, wave=R.ramp_wave):
    o = R.OPS[name]
    return R.model(o, wave(), KH << 32)[0]


def col(out, i=0):
    return [int(v) for v in out[:, i]]


def test_every_op_number_is_taken_once():
    assert sorted(o.num for o in R.OPS.values()) == list(range(R.N_OPS))


# a0[l] = 1000 + l, a1[l] = -7 - l (a2 = 2000 + 3 l, a3 = -3000 + 5 l); "falling": a0[l] = 1000 - l
HAND = {
    "wave_shr1": [-7] + [999 + l for l in L[1:]],
    "wave_shr1_z": [0] + [999 + l for l in L[1:]],
    "row_shr1_z": [0 if l % 16 == 0 else 999 + l for l in L],
    "row_shl1_keep": [-7 - l if l % 16 == 15 else 1001 + l for l in L],
    "quad_shr1": [1000 + l if l % 4 == 0 else 999 + l for l in L],
    "slot_shr1_z<16>": [0 if l in (0, 16, 32, 48) else 999 + l for l in L],
    "slot_shr1_z<32>": [0 if l in (0, 32) else 999 + l for l in L],
    "slot_shr1_z<64>": [0 if l == 0 else 999 + l for l in L],
    "slot_shl1_keep<16>": [-7 - l if l in (15, 31, 47, 63) else 1001 + l for l in L],
    "slot_shl1_keep<32>": [{31: -38, 63: -70}.get(l, 1001 + l) for l in L],
    "slot_shl1_keep<64>": [1001 + l for l in L[:63]] + [-70],
    "row_bcast<0>": [1000 + 16 * (l // 16) for l in L],
    "row_bcast<15>": [1015 + 16 * (l // 16) for l in L],
    "row_bcast<7>": [1007 + 16 * (l // 16) for l in L],
    "slot_bcast<0>": [1000] * 16 + [1016] * 16 + [1032] * 16 + [1048] * 16,
    "slot_bcast<15>": [1015] * 16 + [1031] * 16 + [1047] * 16 + [1063] * 16,
    "slot_bcast<3>": [1003] * 16 + [1019] * 16 + [1035] * 16 + [1051] * 16,
    "slot_first<16>": [1000] * 16 + [1016] * 16 + [1032] * 16 + [1048] * 16,
    "slot_first<32>": [1000] * 32 + [1032] * 32,
    "slot_first<64>": [1000] * 64,
    "slot_last<16>": [1015] * 16 + [1031] * 16 + [1047] * 16 + [1063] * 16,
    "slot_last<32>": [1031] * 32 + [1063] * 32,
    "slot_last<64>": [1063] * 64,
    "set_lane0": [KH] + [1000 + l for l in L[1:]],
    "add_shr1": [-7] + [992] * 63,
    "add_row_shr1": [-7 - l if l % 16 == 0 else 992 for l in L],
    "wave_prefix_max": [1000 + l for l in L],
    "wave_prefix_max16": [1000 + l for l in L],
    "wave_prefix_max32": [1000 + l for l in L],
    "quad_prefix_max": [1000 + l for l in L],
    "quad_all_max": [1003 + 4 * (l // 4) for l in L],
    "max_lanes<16>": [1015] * 64,
    "max_lanes<32>": [1031] * 64,
    "max_lanes<64>": [1063] * 64,
    "wave_max": [1063] * 64,
    "wave_min": [1000] * 64,
}
HAND_FALLING = {
    "wave_prefix_max": [1000] * 64,
    "wave_prefix_max16": [1000] * 16 + [984] * 16 + [968] * 16 + [952] * 16,
    "wave_prefix_max32": [1000] * 32 + [968] * 32,          # the first value of each half
    "quad_prefix_max": [1000 - 4 * (l // 4) for l in L],
    "quad_all_max": [1000 - 4 * (l // 4) for l in L],
    "max_lanes<16>": [1000] * 64,
    "wave_max": [1000] * 64,
    "wave_min": [937] * 64,
    "wave_shr1": [-7] + [1001 - l for l in L[1:]],
    "slot_shl1_keep<32>": [{31: 24, 63: 56}.get(l, 999 - l) for l in L],
}


@pytest.mark.parametrize("name", sorted(HAND))
def test_known_answers_on_the_rising_ramp(name):
    assert col(ramp(name)) == HAND[name]


@pytest.mark.parametrize("name", sorted(HAND_FALLING))
def test_known_answers_on_the_falling_ramp(name):
    assert col(ramp(name, R.falling_wave)) == HAND_FALLING[name]


def test_known_answers_with_more_than_one_word():
    q = ramp("quad_bcast<0..3>")
    for l in L:
        b = 4 * (l // 4)
        assert [int(v) for v in q[l]] == [1000 + b, -7 - (b + 1), 2000 + 3 * (b + 2), -3000 + 5 * (b + 3)]
    for ln in (0, 31, 63):
        p = ramp(f"park/unpark<{ln}>")
        assert col(p, 0) == [KH if l == ln else 1000 + l for l in L] and col(p, 1) == [KH] * 64
    # first8_max2: a = {1000 + l, 0}: the first eight entries are lanes 0 .. 3, both halves -> 1003; b = {-7 - l, -1} -> -1
    f = ramp("first8_max2")
    assert col(f, 0) == [1003] * 64 and col(f, 1) == [-1] * 64
    # quad_shl1_keep8 with the kernels' mask (quad lane 3): register 0 of the first four: src = a0 = 1000 + l, last = a1 + 1 = -6 - l
    o = R.OPS["quad_shl1_keep8 (d)"]
    d = R.model(o, R.ramp_wave(), R.MASK3)[0]
    assert col(d, 0) == [-6 - l if l % 4 == 3 else 1001 + l for l in L]
    r = R.model(R.OPS["quad_shl1_keep8 (r)"], R.ramp_wave(), R.MASK3)[0]     # src = ~a0 = -1001 - l, last = a2 - 1 = 1999 + 3 l
    assert col(r, 0) == [1999 + 3 * l if l % 4 == 3 else -1002 - l for l in L]
    s = R.model(R.OPS["sel_mask"], R.ramp_wave(), 0xAAAAAAAAAAAAAAAA)[0]
    assert col(s) == [1000 + l if l % 2 else -7 - l for l in L]


def one_lane(name, a, k=0):
    arr = np.zeros((1, 64, 4), np.int64)
    arr[0, 0, :len(a)] = a
    return [int(v) for v in R.model(R.OPS[name], arr, k)[0, 0]]


def test_known_answers_of_the_lane_local_ops():
    P = lambda l, h: int(R.pack(l, h))
    assert one_lane("adds", [P(32767, -32768), P(1, -1)]) == [P(32767, -32768)]
    assert one_lane("adds", [P(100, -100), P(-1, 1)]) == [P(99, -99)]
    assert one_lane("subs", [P(-32768, 32767), P(1, -1)]) == [P(-32768, 32767)]
    assert one_lane("vmax", [P(-1, 1), P(0, -32768)]) == [P(0, 1)]
    assert one_lane("vmaxu", [P(-1, 1), P(0, -32768)]) == [P(-1, -32768)]
    assert one_lane("neq01", [P(5, 7), P(5, 8)]) == [0x00010000]
    assert one_lane("eq01", [P(5, 7), P(5, 8)]) == [0x00000001]
    assert one_lane("sign_bits", [P(-5, 7)]) == [0x00008000]
    assert one_lane("bfi", [0x12345678, 0x0abcdef0], 0xffff0000 << 32) == [0x1234def0]
    assert one_lane("pk_mul", [P(3, 0x4000)], P(257, 4) << 32) == [P(771, 0)]
    assert one_lane("pk_mad", [P(3, 5), P(10, -20)], P(2, 3) << 32) == [P(16, -5)]
    assert one_lane("pk_mad_k<8>", [P(1, 0x2000), P(1, 7)]) == [P(9, 7)]
    assert one_lane("adds_lo", [P(-32000, 999)], (P(-4, -1000) & 0xffffffff) << 32) == [P(-32004, -32768)]
    assert one_lane("max_hi_lo", [P(3, -9), P(-2, 100)]) == [P(3, -2)]
    assert one_lane("splat_lo", [P(3, -9)]) == [P(3, 3)] and one_lane("splat_hi", [P(3, -9)]) == [P(-9, -9)]
    cells = [P(0, 1), P(2, 3), P(4, 5), P(6, 7)]
    assert one_lane("cells_split", cells) == [P(0, 4), P(1, 5), P(2, 6), P(3, 7)]
    assert one_lane("cells_join", [P(0, 4), P(1, 5), P(2, 6), P(3, 7)]) == cells
    assert one_lane("clamp16", [32768]) == [32767] and one_lane("sat16", [-40000]) == [-32768] and one_lane("clamp16", [-5]) == [-5]
    assert one_lane("ffbl_u32", [0x00a0]) == [5] and one_lane("ffbl_u32", [0]) == [-1] and one_lane("ffbl_u32", [-(1 << 31)]) == [31]
    assert one_lane("nuc_col_offsets", [0x0f070301]) == [0x1c1c0c04]
    assert one_lane("nuc_keys2", [0x04030201]) == [P((1 << 9) | (2 << 5), (3 << 9) | (4 << 5))]
    assert one_lane("add_word", [P(-1, 2), 10]) == [65545, 12]
    assert one_lane("add_byte", [0x80030201, 10]) == [11, 12, 13, 138]
    assert one_lane("pk", [0x12345, -2]) == [P(0x2345, -2)] and one_lane("splat", [-3]) == [P(-3, -3)]
    assert one_lane("scan8_inreg", [P(10, -50)], (P(-5, -5) & 0xffffffff) << 32) == [P(10, 5)]


@pytest.mark.parametrize("name", list(R.OPS))
def test_the_gpu_inputs_separate_each_helper_from_its_neighbours(name):
    o = R.OPS[name]
    assert o.variants, name
    cases = R.cases_of(o)
    want = [R.model(o, a, k) for a, k in cases]
    for vname, variant in o.variants.items():
        differs = False
        for (a, k), w in zip(cases, want):
            got = R.i32(np.asarray(variant(a, k), np.int64))
            assert got.shape == w.shape, (name, vname, got.shape)
            if (got != w).any():
                differs = True
                break
        assert differs, f"the inputs of {name} do not tell it from: {vname}"


def test_the_named_mistakes_are_among_the_variants():
    """the kinds of confusion the inputs are held against, each present where it applies"""
    for w in (16, 32, 64):
        for fam in ("slot_shr1_z", "slot_shl1_keep", "slot_first", "slot_last"):
            v = R.OPS[f"{fam}<{w}>"].variants
            assert all(f"width {o}" in v for o in (16, 32, 64) if o != w), (fam, w)
    for name in ("wave_shr1", "row_shr1_z", "row_shl1_keep", "slot_shr1_z<32>", "slot_shl1_keep<32>"):
        v = R.OPS[name].variants
        assert "the other direction" in v and ("zero at the edge" in v or "second operand at the edge" in v)
    assert "mirrored source" in R.OPS["slot_first<32>"].variants and "mirrored source" in R.OPS["slot_last<32>"].variants
    assert "high half" in R.OPS["splat_lo"].variants and "low half" in R.OPS["splat_hi"].variants
    assert "unsigned" in R.OPS["vmax"].variants and "signed" in R.OPS["vmaxu"].variants and "unsigned maximum" in R.OPS["wave_prefix_max"].variants
    assert "wrapping" in R.OPS["adds"].variants and "wrapping" in R.OPS["subs"].variants
    assert {"cells_join", "identity"} <= set(R.OPS["cells_split"].variants) and {"cells_split", "identity"} <= set(R.OPS["cells_join"].variants)


def test_inputs_are_what_the_gpu_test_promises():
    a = R.lane_inputs()
    assert a.shape == (260, 64, 4) and np.abs(a[2:258]).max() <= 1 << 30 and a.min() > -(1 << 31)
    assert all(abs(int(a[w, ln, 0])) == R.I32_MAX for w in (258, 259) for ln in R.EDGE_LANES)
    p = R.packed_inputs().reshape(-1, 4)
    seen = {(int(R.lo(r[0])), int(R.hi(r[0])), int(R.lo(r[1])), int(R.hi(r[1]))) for r in p[:15 ** 4]}
    assert len(seen) == 15 ** 4 and p.shape[0] % 64 == 0 and p.shape[0] >= 15 ** 4 + 65536
    b = R.bit_inputs()[..., 0].reshape(-1)
    assert {1 << i for i in range(32)} <= {int(R.u32(v)) for v in b} and 0 in b
    assert set(R.MULS) == {0, 1, 2, 3, 255, 257, 0x8001} and len(R.KH_PAIRS) == 49
    assert {0, 0xffffffffffffffff, 1, 1 << 63, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555} <= set(R.MASKS)


@pytest.mark.parametrize("family", R.KEY_FAMILIES)
def test_key_families(family):
    k = R.sort_keys(family, 1000)
    assert k.dtype == np.uint64 and k.shape == (1000,)
    s, lb = R.sort_expected(k)
    assert (s[lb.astype(np.int64)] == k).all() and (np.diff(s.astype(object)) >= 0).all()
    if family == "distinct":
        assert len(set(k.tolist())) == 1000
    if family == "equal":
        assert len(set(k.tolist())) == 1 and (lb == 0).all()
    if family == "duplicates":
        assert len(set(k.tolist())) < 100
    if family == "sorted":
        assert (k == s).all()
    if family == "reversed":
        assert (k == s[::-1]).all()
    if family == "low words":
        assert len(set((k >> np.uint64(32)).tolist())) == 1 and len(set(k.tolist())) > 900
    if family == "high words":
        assert len(set((k & np.uint64(0xffffffff)).tolist())) == 1 and len(set(k.tolist())) > 900
    if family == "with NO_KEY":
        assert 200 < int((k == np.uint64(R.NO_KEY)).sum()) < 400
