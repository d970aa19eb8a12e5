"""Plain NumPy models of the device helpers that `k_prim_kat` (ba_kernels.hip) runs one by one, the inputs the GPU test feeds them, and for every
helper the mistakes it could be confused with (`variants`), which those inputs must tell apart (tests/test_lane_prims_ref.py, without a GPU).

Every model is written from the comment that documents the helper in ba_device.hpp / ba_quad.hpp / ba_multi.hpp / ba_small.hpp / ba_driver.hpp, not
from its instruction: an index expression over a `[waves, 64]` array, or 16-bit arithmetic carried out in int64 with explicit clipping or wrapping.
A model takes `a` (int64 `[waves, 64, 4]`, every entry an int32 value: the helper's operands a0 .. a3 of each lane) and the wave-uniform 64-bit `k`
(low word `kl`, high word `kh`), and returns int64 `[waves, 64, n_out]` with int32 values: the words the kernel writes.
"""
import functools
from collections import namedtuple

import numpy as np

LANE = np.arange(64)
I32_MAX = (1 << 31) - 1


# ------------------------------------------------------------------ number formats
def i32(v):
    v = np.asarray(v, np.int64) & 0xffffffff
    return np.where(v >= 1 << 31, v - (1 << 32), v)


def u32(v):
    return np.asarray(v, np.int64) & 0xffffffff


def s16(v):
    v = np.asarray(v, np.int64) & 0xffff
    return np.where(v >= 0x8000, v - 0x10000, v)


def lo(v):
    return s16(u32(v))


def hi(v):
    return s16(u32(v) >> 16)


def ulo(v):
    return u32(v) & 0xffff


def uhi(v):
    return u32(v) >> 16


def pack(l, h):
    return i32((np.asarray(l, np.int64) & 0xffff) | ((np.asarray(h, np.int64) & 0xffff) << 16))


def sat(v):
    return np.clip(np.asarray(v, np.int64), -32768, 32767)


def kl_of(k):
    return int(i32(k & 0xffffffff))


def kh_of(k):
    return int(i32((k >> 32) & 0xffffffff))


def per_half(f, *xs):
    """f on the low halves and on the high halves, both as signed 16-bit values; the results' low 16 bits packed"""
    return pack(f(*[lo(x) for x in xs]), f(*[hi(x) for x in xs]))


# ------------------------------------------------------------------ lanes
def shift_down(a, width, edge):
    """lane l <- a[l - 1] inside slots of `width` lanes; a slot's first lane <- edge[l]"""
    return np.where(LANE % width == 0, edge, np.roll(a, 1, axis=1))


def shift_up(a, width, edge):
    """lane l <- a[l + 1] inside slots of `width` lanes; a slot's last lane <- edge[l]"""
    return np.where(LANE % width == width - 1, edge, np.roll(a, -1, axis=1))


def bcast(a, width, src):
    """lane `src` of every slot of `width` lanes, to all lanes of the slot"""
    return a[:, (LANE // width) * width + src]


def prefix_max(a, width):
    """inclusive maximum over the lanes before and at l, restarting every `width` lanes"""
    return np.maximum.accumulate(a.reshape(a.shape[0], 64 // width, width), axis=2).reshape(a.shape)


def first_lanes_max(a, n):
    """the maximum of lanes 0 .. n - 1, in every lane"""
    return np.broadcast_to(a[:, :n].max(axis=1, keepdims=True), a.shape)


def lane_bit(m):
    m = int(m) & 0xffffffffffffffff
    return np.array([(m >> l) & 1 for l in range(64)], bool)[None, :]


def one(x):
    return np.asarray(x, np.int64)[..., None]


def many(*xs):
    return np.stack([np.broadcast_to(np.asarray(x, np.int64), xs[0].shape) for x in xs], axis=-1)


def cells_of(a):
    """the eight 16-bit cells of a lane's four registers, register k = (low, high)"""
    return [h(a[..., r]) for r in range(4) for h in (lo, hi)]


# ------------------------------------------------------------------ the models, one per op of k_prim_kat's switch
Op = namedtuple("Op", "num name kind model n_out variants ks")
OPS = {}
KH = 0x01234567          # the high word of k where an op parks or writes it
KL_HAZARD = 0x5a5a1234   # a second low word: the operands are then x ^ kl with a non-trivial kl


def op(num, name, kind, model, n_out=1, variants=None, ks=None):
    assert name not in OPS and num not in [o.num for o in OPS.values()]
    OPS[name] = Op(num, name, kind, model, n_out, variants or {}, ks)


def A(i):
    return lambda a: a[..., i]


a0, a1, a2, a3 = A(0), A(1), A(2), A(3)

# ---- shifts. `fill` / `last`: the second operand, taken at the edge lane itself
WIDTHS = (4, 16, 32, 64)


def down(width, edge):
    return lambda a, k: one(shift_down(a0(a), width, edge(a)))


def up(width, edge):
    return lambda a, k: one(shift_up(a0(a), width, edge(a)))


def zero(a):
    return 0


def shift_variants(maker, other, width, edge):
    v = {f"width {w}": maker(w, edge) for w in WIDTHS if w != width}
    v["the other direction"] = other(width, edge)
    for name, e in (("zero at the edge", zero), ("own value at the edge", a0), ("second operand at the edge", a1)):
        if e is not edge:
            v[name] = maker(width, e)
    v["no shift"] = lambda a, k: one(a0(a))
    return v


op(0, "wave_shr1", "lane", down(64, a1), variants=shift_variants(down, up, 64, a1))                # lane l <- lane l-1; lane 0 <- fill
op(1, "wave_shr1_z", "lane", down(64, zero), variants=shift_variants(down, up, 64, zero))          # ... lane 0 <- 0
op(2, "row_shr1_z", "lane", down(16, zero), variants=shift_variants(down, up, 16, zero))           # inside the row; row lane 0 <- 0
op(3, "row_shl1_keep", "lane", up(16, a1), variants=shift_variants(up, down, 16, a1))              # lane l <- src[l+1] inside the row; lane 15 keeps `last`
op(4, "quad_shr1", "lane", down(4, a0), variants=shift_variants(down, up, 4, a0))                  # inside the quad; quad lane 0 keeps its own value
for n, w in ((5, 16), (6, 32), (7, 64)):
    op(n, f"slot_shr1_z<{w}>", "lane", down(w, zero), variants=shift_variants(down, up, w, zero))  # inside the slot; its first lane <- 0
for n, w in ((8, 16), (9, 32), (10, 64)):
    op(n, f"slot_shl1_keep<{w}>", "lane", up(w, a1), variants=shift_variants(up, down, w, a1))     # src[l+1] inside the slot; its last lane keeps `last`


# ---- broadcasts
def bc(width, src):
    return lambda a, k: one(bcast(a0(a), width, src))


def bcast_variants(width, src):
    v = {}
    for w in WIDTHS:
        if w != width:
            v[f"width {w}"] = bc(w, 0 if src == 0 else (w - 1 if src == width - 1 else min(src, w - 1)))
    v["mirrored source"] = bc(width, width - 1 - src)
    v["next source"] = bc(width, (src + 1) % width)
    v["previous source"] = bc(width, (src - 1) % width)
    v["no broadcast"] = lambda a, k: one(a0(a))
    return v


op(11, "row_bcast<0>", "lane", bc(16, 0), variants=bcast_variants(16, 0))
op(12, "row_bcast<15>", "lane", bc(16, 15), variants=bcast_variants(16, 15))
op(13, "row_bcast<7>", "lane", bc(16, 7), variants=bcast_variants(16, 7))
op(14, "slot_bcast<0>", "lane", bc(16, 0), variants=bcast_variants(16, 0))     # lane SRC (0..15) of every 16-lane slot to all lanes of the slot
op(15, "slot_bcast<15>", "lane", bc(16, 15), variants=bcast_variants(16, 15))
op(16, "slot_bcast<3>", "lane", bc(16, 3), variants=bcast_variants(16, 3))


def quad_bcasts(order):
    return lambda a, k: many(*[bcast(a[..., i], 4, order[i]) for i in range(4)])


op(17, "quad_bcast<0..3>", "lane", quad_bcasts((0, 1, 2, 3)), n_out=4,
   variants={"mirrored sources": quad_bcasts((3, 2, 1, 0)), "all from lane 0": quad_bcasts((0, 0, 0, 0)), "rotated sources": quad_bcasts((1, 2, 3, 0)),
             "row lanes": lambda a, k: many(*[bcast(a[..., i], 16, i) for i in range(4)]), "no broadcast": lambda a, k: a})
for n, w in ((18, 16), (19, 32), (20, 64)):
    op(n, f"slot_first<{w}>", "lane", bc(w, 0), variants=bcast_variants(w, 0))          # the slot's first lane's value, to all its lanes
for n, w in ((21, 16), (22, 32), (23, 64)):
    op(n, f"slot_last<{w}>", "lane", bc(w, w - 1), variants=bcast_variants(w, w - 1))   # the slot's last lane's value, to all its lanes


def write_lane(a, lane, val):
    return np.where(LANE == lane, val, a)


def parked(lane):
    def f(a, k):
        return many(write_lane(a0(a), lane, kh_of(k)), kh_of(k))   # the register with the value parked in lane LANE, and what unpark reads back
    return f


op(24, "set_lane0", "lane", lambda a, k: one(write_lane(a0(a), 0, kh_of(k))),        # write a wave-uniform value into lane 0 of v
   variants={"lane 1": lambda a, k: one(write_lane(a0(a), 1, kh_of(k))), "lane 63": lambda a, k: one(write_lane(a0(a), 63, kh_of(k))),
             "every lane": lambda a, k: one(0 * a0(a) + kh_of(k)), "nothing written": lambda a, k: one(a0(a)),
             "the low word of k": lambda a, k: one(write_lane(a0(a), 0, kl_of(k)))})
for n, ln in ((25, 0), (26, 31), (27, 63)):
    op(n, f"park/unpark<{ln}>", "lane", parked(ln), n_out=2,
       variants={"lane %d" % o: parked(o) for o in (0, 1, 30, 31, 32, 62, 63) if o != ln} |
                {"unpark reads the lane's old value": lambda a, k, ln=ln: many(write_lane(a0(a), ln, kh_of(k)), a0(a)[:, ln:ln + 1])})


# ---- adds, maxima and scans over lanes
def add_down(width):
    return lambda a, k: one(i32(shift_down(a0(a), width, 0) + a1(a)))   # a[l-1] + b[l] (first lane: 0 + b)


def add_variants(width):
    v = {f"width {w}": add_down(w) for w in WIDTHS if w != width}
    v["the other direction"] = lambda a, k: one(i32(shift_up(a0(a), width, 0) + a1(a)))
    v["own value at the edge"] = lambda a, k: one(i32(shift_down(a0(a), width, a0(a)) + a1(a)))
    v["no shift"] = lambda a, k: one(i32(a0(a) + a1(a)))
    v["b shifted, not a"] = lambda a, k: one(i32(a0(a) + shift_down(a1(a), width, 0)))
    v["difference"] = lambda a, k: one(i32(shift_down(a0(a), width, 0) - a1(a)))
    return v


op(28, "add_shr1", "lane", add_down(64), variants=add_variants(64))
op(29, "add_row_shr1", "lane", add_down(16), variants=add_variants(16))


def pmax(width, conv=lambda x: x):
    return lambda a, k: one(i32(prefix_max(conv(a0(a)), width)))


def pmax_variants(width):
    v = {f"width {w}": pmax(w) for w in WIDTHS if w != width}
    v["unsigned maximum"] = pmax(width, u32)
    v["exclusive"] = lambda a, k: one(shift_down(prefix_max(a0(a), width), width, a0(a)))
    v["minimum"] = lambda a, k: one(-prefix_max(-a0(a), width))
    v["suffix maximum"] = lambda a, k: one(prefix_max(a0(a)[:, ::-1], width)[:, ::-1])
    return v


op(30, "wave_prefix_max", "lane", pmax(64), variants=pmax_variants(64))        # inclusive prefix max over the 64 lanes
op(31, "wave_prefix_max16", "lane", pmax(16), variants=pmax_variants(16))      # ... restarting every 16 lanes (multi_carry<16>: four slots)
op(32, "wave_prefix_max32", "lane", pmax(32), variants=pmax_variants(32))      # ... every 32 lanes (multi_carry<32>: two slots)


def fmax(n, conv=lambda x: x):
    return lambda a, k: one(i32(first_lanes_max(conv(a0(a)), n)))


def fmax_variants(n):
    v = {f"{w} lanes": fmax(w) for w in (4, 15, 16, 31, 32, 63, 64) if w != n}
    v["unsigned maximum"] = fmax(n, u32)
    v["minimum"] = lambda a, k: one(-first_lanes_max(-a0(a), n))
    v["per slot"] = lambda a, k: one(bcast(prefix_max(a0(a), n), n, n - 1)) if n < 64 else one(a0(a))
    return v


for n, w in ((33, 16), (34, 32), (35, 64)):
    op(n, f"max_lanes<{w}>", "lane", fmax(w), variants=fmax_variants(w))       # the maximum of the first LANES lanes, wave-uniform
op(36, "wave_max", "lane", fmax(64), variants=fmax_variants(64))
op(37, "wave_min", "lane", lambda a, k: one(-first_lanes_max(-a0(a), 64)),
   variants={"maximum": fmax(64), "unsigned minimum": lambda a, k: one(i32(-first_lanes_max(-u32(a0(a)), 64))),
             "32 lanes": lambda a, k: one(-first_lanes_max(-a0(a), 32)), "63 lanes": lambda a, k: one(-first_lanes_max(-a0(a), 63))})


def first_entries_max(lanes, halves=(lo, hi), conv=lambda x: x):
    def f(a, k):
        def m(x):
            return first_lanes_max(np.maximum.reduce([conv(h(x)) for h in halves]), lanes)
        return many(m(a0(a)), m(a1(a)))
    return f


op(38, "first8_max2", "lane", first_entries_max(4), n_out=2,                    # max of the first 8 entries (lanes 0..3, both halves) of two packed registers
   variants={"first 6 entries": first_entries_max(3), "first 10 entries": first_entries_max(5), "first 4 entries": first_entries_max(2),
             "first 16 entries": first_entries_max(8), "low halves only": first_entries_max(4, (lo,)), "high halves only": first_entries_max(4, (hi,)),
             "unsigned maximum": lambda a, k: many(*[s16(first_lanes_max(np.maximum(ulo(x), uhi(x)), 4)) for x in (a0(a), a1(a))]),
             "a and b exchanged": lambda a, k: first_entries_max(4)(a, k)[..., ::-1]})
op(39, "quad_prefix_max", "lane", pmax(4), variants=pmax_variants(4))          # inclusive prefix max inside every quad


def qmax(width, conv=lambda x: x):
    return lambda a, k: one(i32(bcast(prefix_max(conv(a0(a)), width), width, width - 1)))


op(40, "quad_all_max", "lane", qmax(4),                                        # max over the quad, in every lane
   variants={"width 16": qmax(16), "width 64": qmax(64), "unsigned maximum": qmax(4, u32), "prefix maximum": pmax(4),
             "pairs": lambda a, k: one(bcast(prefix_max(a0(a), 2), 2, 1))})


def quad_shl8(which, width=4, own=False, shift=shift_up):
    """lane l <- mask bit l ? last[l] : src[l + 1] inside the quad (the caller's mask names quad lane 3, whose source is itself), for the eight
    registers src = (a, ~a), last = (a rotated by one register + 1, a rotated by two - 1) that k_prim_kat builds; which: 0 the first four, 1 the rest"""
    def f(a, k):
        outs = []
        for r in range(4):
            src = a[..., r] if which == 0 else i32(~a[..., r])
            last = i32(a[..., (r + 1) % 4] + 1) if which == 0 else i32(a[..., (r + 2) % 4] - 1)
            outs.append(np.where(lane_bit(k), src if own else last, shift(src, width, src)))
        return many(*outs)
    return f


MASK3 = 0x8888888888888888
for n, which in ((41, 0), (42, 1)):
    op(n, "quad_shl1_keep8 (%s)" % ("d" if which == 0 else "r"), "lane", quad_shl8(which), n_out=4,
       variants={"the other four registers": quad_shl8(1 - which), "own value where the mask is set": quad_shl8(which, own=True),
                 "mask ignored": lambda a, k, which=which: quad_shl8(which)(a, 0),
                 "shift down": quad_shl8(which, shift=shift_down)},
       ks=[MASK3, ~0 & 0xffffffffffffffff, MASK3 | 0x0123456789abcdef, MASK3 | 0x1111111111111111])

# ---- packed 16-bit and bit arithmetic inside the lane
V15 = (-32768, -32767, -16385, -16384, -2, -1, 0, 1, 2, 255, 256, 16383, 16384, 32766, 32767)


def local(f):
    return lambda a, k: one(f(a0(a), a1(a), k))


op(43, "adds", "packed", local(lambda x, y, k: per_half(lambda p, q: sat(p + q), x, y)),
   variants={"wrapping": local(lambda x, y, k: per_half(lambda p, q: p + q, x, y)), "32-bit add": local(lambda x, y, k: i32(x + y)),
             "unsigned saturation": local(lambda x, y, k: pack(np.minimum(ulo(x) + ulo(y), 65535), np.minimum(uhi(x) + uhi(y), 65535))),
             "subs": local(lambda x, y, k: per_half(lambda p, q: sat(p - q), x, y))})
op(44, "subs", "packed", local(lambda x, y, k: per_half(lambda p, q: sat(p - q), x, y)),
   variants={"wrapping": local(lambda x, y, k: per_half(lambda p, q: p - q, x, y)), "32-bit subtract": local(lambda x, y, k: i32(x - y)),
             "operands exchanged": local(lambda x, y, k: per_half(lambda p, q: sat(q - p), x, y)),
             "unsigned saturation": local(lambda x, y, k: pack(np.maximum(ulo(x) - ulo(y), 0), np.maximum(uhi(x) - uhi(y), 0)))})
op(45, "vmax", "packed", local(lambda x, y, k: per_half(np.maximum, x, y)),
   variants={"unsigned": local(lambda x, y, k: pack(np.maximum(ulo(x), ulo(y)), np.maximum(uhi(x), uhi(y)))), "32-bit maximum": local(lambda x, y, k: np.maximum(x, y)),
             "minimum": local(lambda x, y, k: per_half(np.minimum, x, y))})
op(46, "vmaxu", "packed", local(lambda x, y, k: pack(np.maximum(ulo(x), ulo(y)), np.maximum(uhi(x), uhi(y)))),
   variants={"signed": local(lambda x, y, k: per_half(np.maximum, x, y)), "32-bit unsigned maximum": local(lambda x, y, k: i32(np.maximum(u32(x), u32(y)))),
             "minimum": local(lambda x, y, k: pack(np.minimum(ulo(x), ulo(y)), np.minimum(uhi(x), uhi(y))))})


def neq(x, y, k):
    return per_half(lambda p, q: (p != q).astype(np.int64), x, y)    # per 16-bit half: 1 where a != b, else 0


def eq(x, y, k):
    return per_half(lambda p, q: (p == q).astype(np.int64), x, y)    # per 16-bit half: 1 where a == b, else 0


CMP_VARIANTS = {"low half's answer in both": lambda f: local(lambda x, y, k: pack(lo(f(x, y, k)), lo(f(x, y, k)))),
                "high half's answer in both": lambda f: local(lambda x, y, k: pack(hi(f(x, y, k)), hi(f(x, y, k)))),
                "whole register compared": lambda f: local(lambda x, y, k: pack(((x != y) == (f is neq)).astype(np.int64), ((x != y) == (f is neq)).astype(np.int64))),
                "high half always 0": lambda f: local(lambda x, y, k: pack(lo(f(x, y, k)), 0)),
                "signed difference clipped at 1": lambda f: local(lambda x, y, k: per_half(lambda p, q: np.clip(p - q, 0, 1) if f is neq else np.clip(1 - (p - q), 0, 1), x, y))}
op(47, "neq01", "packed", local(neq), variants={"eq01": local(eq)} | {n: v(neq) for n, v in CMP_VARIANTS.items()})
op(48, "eq01", "packed", local(eq), variants={"neq01": local(neq)} | {n: v(eq) for n, v in CMP_VARIANTS.items()})
op(49, "sign_bits", "packed", local(lambda x, y, k: i32(u32(x) & 0x80008000)),    # bit 15 of each half, everything else cleared
   variants={"high half only": local(lambda x, y, k: i32(u32(x) & 0x80000000)), "low half only": local(lambda x, y, k: u32(x) & 0x8000),
             "bits 14": local(lambda x, y, k: u32(x) & 0x40004000), "nothing cleared": local(lambda x, y, k: x)})
MULS = (0, 1, 2, 3, 255, 257, 0x8001)
KH_PAIRS = [(h << 16 | l) << 32 for l in MULS for h in MULS]


def khw(k):
    return u32(kh_of(k))


op(50, "bfi", "packed", local(lambda x, y, k: i32((u32(x) & khw(k)) | (u32(y) & ~khw(k)))),    # (a & mask) | (b & ~mask)
   variants={"a and b exchanged": local(lambda x, y, k: i32((u32(y) & khw(k)) | (u32(x) & ~khw(k)))), "and only": local(lambda x, y, k: i32(u32(x) & khw(k))),
             "or": local(lambda x, y, k: i32(u32(x) & khw(k) | u32(y)))},
   ks=[m << 32 for m in (0, 0xffffffff, 0x80008000, 0xC000C000, 0x0000ffff, 0xffff0000, 0x55555555, 0x9e3779b9)])


def mad(m_of, c_of=lambda x, y: y):
    def f(x, y, k):
        m = m_of(k)
        return pack(lo(x) * ulo(m) + lo(c_of(x, y)), hi(x) * uhi(m) + hi(c_of(x, y)))   # per half: a * m + c (mod 2^16)
    return local(f)


def mad_variants(m_of, c_of=lambda x, y: y, uniform=True):
    v = {"32-bit arithmetic": local(lambda x, y, k: i32(u32(x) * ulo(m_of(k)) + u32(c_of(x, y)))),
         "saturating": local(lambda x, y, k: pack(sat(lo(x) * s16(ulo(m_of(k))) + lo(c_of(x, y))), sat(hi(x) * s16(uhi(m_of(k))) + hi(c_of(x, y))))),
         "a's low half in both": local(lambda x, y, k: pack(lo(x) * ulo(m_of(k)) + lo(c_of(x, y)), lo(x) * uhi(m_of(k)) + hi(c_of(x, y))))}
    if uniform:
        v["multiplier's low half in both"] = mad(lambda k: pack(ulo(m_of(k)), ulo(m_of(k))), c_of)
        v["multiplier's high half in both"] = mad(lambda k: pack(uhi(m_of(k)), uhi(m_of(k))), c_of)
        v["multiplier's halves exchanged"] = mad(lambda k: pack(uhi(m_of(k)), ulo(m_of(k))), c_of)
    return v


op(51, "pk_mul", "packed", mad(kh_of, lambda x, y: 0 * y), variants=mad_variants(kh_of, lambda x, y: 0 * y), ks=KH_PAIRS)
op(52, "pk_mad", "packed", mad(kh_of), variants=mad_variants(kh_of) | {"nothing added": mad(kh_of, lambda x, y: 0 * y)}, ks=KH_PAIRS)
MAD_K = {53: 2, 54: 4, 55: 8, 56: 0, 57: 1, 58: 64}   # the kernels use 2, 4 and 8; 0, 1 and 64 are the ends of the inline constants
for n, mk in MAD_K.items():
    const = lambda k, mk=mk: pack(mk, mk)
    op(n, f"pk_mad_k<{mk}>", "packed", mad(const),
       variants=({} if mk == 0 else mad_variants(const, uniform=False) | {"the constant in the low half only": mad(lambda k, mk=mk: pack(mk, 0))}) | {"nothing added": mad(const, lambda x, y: 0 * y)} |
                {f"M = {o}": mad(lambda k, o=o: pack(o, o)) for o in (0, 1, 2, 3, 4, 8, 16, 32, 63, 64) if o != mk})
GAPS2 = [pack(l, h) for l, h in ((0, 0), (0, -4), (-4, -8), (-1, -2), (-128, -256), (-32768, 32767), (5, -5), (-20000, -30000))]
op(59, "adds_lo", "packed", local(lambda x, y, k: pack(sat(lo(x) + lo(kh_of(k))), sat(lo(x) + hi(kh_of(k))))),   # {a.lo (+) k.lo, a.lo (+) k.hi}, saturating
   variants={"wrapping": local(lambda x, y, k: pack(lo(x) + lo(kh_of(k)), lo(x) + hi(kh_of(k)))),
             "a's high half for the high half": local(lambda x, y, k: pack(sat(lo(x) + lo(kh_of(k))), sat(hi(x) + hi(kh_of(k))))),
             "a's high half in both": local(lambda x, y, k: pack(sat(hi(x) + lo(kh_of(k))), sat(hi(x) + hi(kh_of(k))))),
             "k's low half in both": local(lambda x, y, k: pack(sat(lo(x) + lo(kh_of(k))), sat(lo(x) + lo(kh_of(k))))),
             "k's halves exchanged": local(lambda x, y, k: pack(sat(lo(x) + hi(kh_of(k))), sat(lo(x) + lo(kh_of(k)))))},
   ks=[int(u32(g)) << 32 for g in GAPS2])
op(60, "max_hi_lo", "packed", local(lambda x, y, k: pack(lo(x), np.maximum(hi(x), lo(y)))),    # {a.lo, max(a.hi, b.lo)}
   variants={"b's high half": local(lambda x, y, k: pack(lo(x), np.maximum(hi(x), hi(y)))), "into the low half": local(lambda x, y, k: pack(np.maximum(lo(x), lo(y)), hi(x))),
             "a's low half against b's": local(lambda x, y, k: pack(lo(x), np.maximum(lo(x), lo(y)))), "unsigned": local(lambda x, y, k: pack(lo(x), np.maximum(uhi(x), ulo(y)))),
             "low half cleared": local(lambda x, y, k: pack(0, np.maximum(hi(x), lo(y)))), "both halves": local(lambda x, y, k: per_half(np.maximum, x, y)),
             "minimum": local(lambda x, y, k: pack(lo(x), np.minimum(hi(x), lo(y))))})
SPLAT_LO, SPLAT_HI = local(lambda x, y, k: pack(lo(x), lo(x))), local(lambda x, y, k: pack(hi(x), hi(x)))
IDENT = local(lambda x, y, k: x)
SWAP = local(lambda x, y, k: pack(hi(x), lo(x)))
op(61, "splat_lo", "packed", SPLAT_LO, variants={"high half": SPLAT_HI, "identity": IDENT, "halves exchanged": SWAP})
op(62, "splat_hi", "packed", SPLAT_HI, variants={"low half": SPLAT_LO, "identity": IDENT, "halves exchanged": SWAP})
op(63, "scan8_splat_lo", "packed", SPLAT_LO, variants={"high half": SPLAT_HI, "identity": IDENT, "halves exchanged": SWAP})
op(64, "scan8_splat_hi", "packed", SPLAT_HI, variants={"low half": SPLAT_LO, "identity": IDENT, "halves exchanged": SWAP})
MASKS = [0, 0xffffffffffffffff, 1, 1 << 63, 0xAAAAAAAAAAAAAAAA, 0x5555555555555555, 0x9e3779b97f4a7c15, 0x0123456789abcdef]
op(65, "sel_mask", "lane", lambda a, k: one(np.where(lane_bit(k), a0(a), a1(a))),      # mask bit set ? a : b
   variants={"a and b exchanged": lambda a, k: one(np.where(lane_bit(k), a1(a), a0(a))),
             "the mask's words exchanged": lambda a, k: one(np.where(lane_bit(((k >> 32) | (k << 32)) & 0xffffffffffffffff), a0(a), a1(a))),
             "the low word for both halves of the wave": lambda a, k: one(np.where(lane_bit((k & 0xffffffff) * 0x100000001), a0(a), a1(a))),
             "the mask's bits mirrored": lambda a, k: one(np.where(lane_bit(k)[:, ::-1], a0(a), a1(a))),
             "always a": lambda a, k: one(a0(a)), "always b": lambda a, k: one(a1(a))},
   ks=MASKS)


def split(a, k):   # (c0 c1)(c2 c3)(c4 c5)(c6 c7) -> (c0 c4)(c1 c5)(c2 c6)(c3 c7)
    c = cells_of(a)
    return many(*[pack(c[r], c[r + 4]) for r in range(4)])


def join(a, k):    # ... and back
    c = cells_of(a)   # register r holds cells (r, r + 4): c[2r] = cell r, c[2r + 1] = cell r + 4
    cell = {r: c[2 * r] for r in range(4)} | {r + 4: c[2 * r + 1] for r in range(4)}
    return many(*[pack(cell[2 * r], cell[2 * r + 1]) for r in range(4)])


op(66, "cells_split", "packed", split, n_out=4, variants={"cells_join": join, "identity": lambda a, k: a,
                                                          "halves exchanged": lambda a, k: many(*[pack(hi(x), lo(x)) for x in np.moveaxis(split(a, k), -1, 0)])})
op(67, "cells_join", "packed", join, n_out=4, variants={"cells_split": split, "identity": lambda a, k: a,
                                                        "halves exchanged": lambda a, k: many(*[pack(hi(x), lo(x)) for x in np.moveaxis(join(a, k), -1, 0)])})
CLAMP_VARIANTS = {"identity": IDENT, "wrapping": local(lambda x, y, k: lo(x)), "unsigned range": local(lambda x, y, k: np.clip(x, 0, 65535)),
                  "symmetric range": local(lambda x, y, k: np.clip(x, -32767, 32767))}
op(68, "clamp16", "packed", local(lambda x, y, k: sat(x)), variants=CLAMP_VARIANTS)
op(69, "sat16", "packed", local(lambda x, y, k: sat(x)), variants=CLAMP_VARIANTS)


def lowest_bit(x, y, k):   # the position of the lowest set bit, 0xffffffff for 0
    x = u32(x)
    low = x & -x
    return np.where(x == 0, -1, np.round(np.log2(np.maximum(low, 1))).astype(np.int64))


def highest_bit(x, y, k):
    x = u32(x)
    return np.where(x == 0, -1, np.floor(np.log2(np.maximum(x, 1))).astype(np.int64))


op(70, "ffbl_u32", "bits", local(lowest_bit),
   variants={"highest set bit": local(highest_bit), "counted from the top": local(lambda x, y, k: np.where(u32(x) == 0, -1, 31 - lowest_bit(x, y, k))),
             "32 for zero": local(lambda x, y, k: np.where(u32(x) == 0, 32, lowest_bit(x, y, k))), "0 for zero": local(lambda x, y, k: np.maximum(lowest_bit(x, y, k), 0)),
             "lowest clear bit": local(lambda x, y, k: lowest_bit(~u32(x), y, k))})


def bytes_of(x):
    return [(u32(x) >> (8 * i)) & 0xff for i in range(4)]


def from_bytes(b):
    return i32(sum((np.asarray(v, np.int64) & 0xff) << (8 * i) for i, v in enumerate(b)))


op(71, "nuc_col_offsets", "packed", local(lambda x, y, k: from_bytes([(b & 7) * 4 for b in bytes_of(x)])),   # byte c -> (c & 7) * 4, the four column bytes at once
   variants={"(c & 15) * 4": local(lambda x, y, k: from_bytes([(b & 15) * 4 for b in bytes_of(x)])), "(c & 7) * 2": local(lambda x, y, k: from_bytes([(b & 7) * 2 for b in bytes_of(x)])),
             "(c & 3) * 4": local(lambda x, y, k: from_bytes([(b & 3) * 4 for b in bytes_of(x)])), "bytes reversed": local(lambda x, y, k: from_bytes([(b & 7) * 4 for b in bytes_of(x)][::-1])),
             "first byte for all": local(lambda x, y, k: from_bytes([(bytes_of(x)[0] & 7) * 4] * 4))})


def keys2(order, letter=15):
    def key_off(p, q):   # nuc_key_off
        return (((p & letter) << 4) | (q & letter)) << 5

    def f(x, y, k):
        b = bytes_of(x)
        return pack(key_off(b[order[0]], b[order[1]]), key_off(b[order[2]], b[order[3]]))   # {a, b, a', b'} bytes -> {key(a, b), key(a', b')} as halves
    return local(f)


op(72, "nuc_keys2", "packed", keys2((0, 1, 2, 3)), variants={"a and b exchanged": keys2((1, 0, 3, 2)), "the pairs exchanged": keys2((2, 3, 0, 1)),
                                                               "the first pair twice": keys2((0, 1, 0, 1)), "interleaved": keys2((0, 2, 1, 3)),
                                                               "three bits a letter": keys2((0, 1, 2, 3), 7)})


def add_part(bits, n, signed=False, order=None):
    def f(a, k):
        x, y = a0(a), a1(a)
        outs = []
        for w in (order or range(n)):
            part = (u32(x) >> (bits * w)) & ((1 << bits) - 1)
            if signed:
                part = np.where(part >= 1 << (bits - 1), part - (1 << bits), part)
            outs.append(i32(part + y))      # base + the chosen word / byte of `packed`, unsigned
        return many(*outs)
    return f


op(73, "add_word", "packed", add_part(16, 2), n_out=2, variants={"signed halves": add_part(16, 2, True), "halves exchanged": add_part(16, 2, order=(1, 0)),
                                                                  "bytes": add_part(8, 2), "the low half both times": add_part(16, 2, order=(0, 0))})
op(74, "add_byte", "packed", add_part(8, 4), n_out=4, variants={"signed bytes": add_part(8, 4, True), "bytes reversed": add_part(8, 4, order=(3, 2, 1, 0)),
                                                                 "halves": lambda a, k: add_part(16, 2, order=(0, 0, 1, 1))(a, k), "byte 0 every time": add_part(8, 4, order=(0, 0, 0, 0))})
op(75, "pk", "packed", local(lambda x, y, k: pack(x, y)), variants={"operands exchanged": local(lambda x, y, k: pack(y, x)), "the first's high half kept": local(lambda x, y, k: i32(u32(x) | (u32(y) << 16))),
                                                                     "high halves": local(lambda x, y, k: pack(hi(x), hi(y)))})
op(76, "splat", "packed", local(lambda x, y, k: pack(x, x)), variants={"identity": IDENT, "high half": SPLAT_HI, "low half only": local(lambda x, y, k: ulo(x))})
GE2 = [int(u32(pack(g, g))) << 32 for g in (0, -1, -5, -128, -32768)]


def inreg(x, y, k):   # inside a register: the second cell against the first's gap (ge2 = the gap cost in both halves, not positive)
    t = sat(lo(x) + lo(kh_of(k)))
    return pack(np.maximum(lo(x), t), np.maximum(hi(x), t))


op(77, "scan8_inreg", "packed", local(inreg),
   variants={"wrapping": local(lambda x, y, k: pack(lo(x), np.maximum(hi(x), s16(lo(x) + lo(kh_of(k)))))),
             "each half against its own gap": local(lambda x, y, k: pack(lo(x), np.maximum(hi(x), sat(hi(x) + lo(kh_of(k)))))),
             "the first cell against the second's": local(lambda x, y, k: pack(np.maximum(lo(x), sat(hi(x) + lo(kh_of(k)))), hi(x))),
             "no gap": local(lambda x, y, k: pack(lo(x), np.maximum(hi(x), lo(x)))), "identity": IDENT},
   ks=GE2)

N_OPS = 78
assert sorted(o.num for o in OPS.values()) == list(range(N_OPS))


# ------------------------------------------------------------------ the inputs of the GPU test
def ramp_wave():
    """the hand-written ramps: a0 = 1000 + l, a1 = -7 - l, a2 = 2000 + 3 l, a3 = -3000 + 5 l"""
    return np.stack([1000 + LANE, -7 - LANE, 2000 + 3 * LANE, -3000 + 5 * LANE], axis=-1).astype(np.int64)[None]


def falling_wave():
    return np.stack([1000 - LANE, -7 + LANE, 2000 - 3 * LANE, -3000 - 5 * LANE], axis=-1).astype(np.int64)[None]


EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)


@functools.lru_cache(maxsize=None)
def lane_inputs():
    """[260, 64, 4]: the two ramps, 256 waves of random int32 within +-2^30, and two waves whose edge lanes hold the extremes (+-(2^31 - 1): wave_min
    negates, INT32_MIN is outside its contract), in alternating order and the second operand against the first"""
    rng = np.random.default_rng(20240607)
    rnd = rng.integers(-(1 << 30), (1 << 30) + 1, (256, 64, 4), dtype=np.int64)
    edges = rng.integers(-1000, 1001, (2, 64, 4), dtype=np.int64)
    for w in range(2):
        for i, ln in enumerate(EDGE_LANES):
            s = 1 if (i + w) % 2 == 0 else -1
            edges[w, ln] = [s * I32_MAX, -s * I32_MAX, s * I32_MAX, -s * I32_MAX]
    return np.concatenate([ramp_wave(), falling_wave(), rnd, edges])


@functools.lru_cache(maxsize=None)
def packed_inputs():
    """[1816, 64, 4]: every combination of low and high halves of a0 and a1 from V15 (15^4 = 50 625 lanes; a2 = a1 with its halves exchanged, a3 = a0 with
    its halves exchanged), 65 536 lanes of random int32, and in the padding to whole waves the values around the int16 range and the ends of int32"""
    v = np.array(V15, np.int64)
    x0l, x0h, x1l, x1h = [g.reshape(-1) for g in np.meshgrid(v, v, v, v, indexing="ij")]
    combos = np.stack([pack(x0l, x0h), pack(x1l, x1h), pack(x1h, x1l), pack(x0h, x0l)], axis=-1)
    rng = np.random.default_rng(20240608)
    rnd = rng.integers(-(1 << 31), 1 << 31, (65536, 4), dtype=np.int64)
    ends = np.array([-(1 << 31), -(1 << 31) + 1, -65537, -65536, -65535, -32770, -32769, -32768, -32767, -1, 0, 1, 32766, 32767, 32768, 32769, 65535, 65536, 65537,
                     I32_MAX - 1, I32_MAX], np.int64)
    pad = np.stack([ends, ends[::-1], ends, ends[::-1]], axis=-1)
    lanes = np.concatenate([combos, rnd, pad])
    fill = (-len(lanes)) % 64
    lanes = np.concatenate([lanes, np.zeros((fill, 4), np.int64)])
    return lanes.reshape(-1, 64, 4)


@functools.lru_cache(maxsize=None)
def bit_inputs():
    """[66, 64, 4]: every single-bit word, zero (the walk passes it: "no such cell"), every word with a single clear bit, and 4096 random words, a
    quarter of them with their low bits cleared"""
    rng = np.random.default_rng(20240609)
    single = [1 << b for b in range(32)]
    first = np.array(single + [0] * 32, np.int64)
    second = np.array([0xffffffff ^ s for s in single] + [0xffffffff << b & 0xffffffff for b in range(32)], np.int64)
    rnd = rng.integers(0, 1 << 32, 4096, dtype=np.int64)
    rnd[:1024] &= 0xffffffff << rng.integers(0, 32, 1024, dtype=np.int64)
    a = i32(np.concatenate([first, second, rnd]))
    return np.stack([a, a[::-1], a, a[::-1]], axis=-1).reshape(-1, 64, 4)


def inputs_of(o):
    return {"lane": lane_inputs, "packed": packed_inputs, "bits": bit_inputs}[o.kind]()


def ks_of(o):
    """the wave-uniform words an op is run with. Cross-lane ops run twice: with kl = 0 and with a kl that makes x ^ kl a real operation on every bit"""
    if o.ks is not None:
        return list(o.ks)
    if o.kind == "lane":
        return [KH << 32, KH << 32 | KL_HAZARD]
    return [0]


def cases_of(o):
    """(a, k) for every launch of the GPU test"""
    return [(inputs_of(o), k) for k in ks_of(o)]


def model(o, a, k):
    out = np.asarray(o.model(a, k), np.int64)
    assert out.shape == a.shape[:2] + (o.n_out,), (o.name, out.shape)
    return i32(out)


# ------------------------------------------------------------------ the sort and the search
NO_KEY = 0xffffffffffffffff
SORT_THREADS = {64: 1024, 1024: 8192}     # THREADS -> the largest count its kernels sort in LDS (SELECT_MAX_PER_READ, SEEDING_SORT_LDS)
SORT_SIZES = (0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 1000, 1023, 1024)
KEY_FAMILIES = ("distinct", "equal", "duplicates", "sorted", "reversed", "low words", "high words", "with NO_KEY")


def sort_sizes(threads):
    cap = SORT_THREADS[threads]
    return sorted(set(SORT_SIZES) | {cap - 1, cap})


def sort_keys(family, n, seed=0):
    rng = np.random.default_rng([20240610, seed, n, KEY_FAMILIES.index(family)])
    rnd = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if family == "distinct":
        return rng.permutation(np.arange(n, dtype=np.uint64) * np.uint64(0x9e3779b97f4a7c15) + np.uint64(12345))   # (odd multiplier: a bijection)
    if family == "equal":
        return np.full(n, 0x0123456789abcdef, np.uint64)
    if family == "duplicates":
        return rnd[rng.integers(0, max(1, n // 16 + 1), n)] if n else rnd
    if family == "sorted":
        return np.sort(rnd)
    if family == "reversed":
        return np.sort(rnd)[::-1].copy()
    if family == "low words":
        return np.uint64(0x00000007 << 32) | (rnd & np.uint64(0xffffffff))
    if family == "high words":
        return (rnd & np.uint64(0xffffffff00000000)) | np.uint64(0x80000001)
    if family == "with NO_KEY":
        return np.where(rng.random(n) < 0.3, np.uint64(NO_KEY), rnd)
    raise ValueError(family)


def sort_expected(keys):
    s = np.sort(keys)
    return s, np.searchsorted(s, keys, side="left").astype(np.uint64)
