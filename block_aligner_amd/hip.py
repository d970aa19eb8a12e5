"""ctypes binding of libblock_aligner_hip.so (include/block_aligner_hip.h) and a host-side mirror of the reference's
Rust API for this path: `PaddedBytes`, `Block` (const-generic modes as constructor flags), `Cigar`, `AlignResult`,
`percent_len` (src/scan_block.rs, src/cigar.rs, src/lib.rs), plus `BatchAligner` over the batch launcher.

There is no CPU fallback: importing works anywhere (so the symbol table can be checked without a GPU), but every
alignment call goes to the HIP kernels and fails loudly if the library or a gfx950 device is missing.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

from . import scores as S

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libblock_aligner_hip.so")

TRACE, X_DROP, LOCAL_START, FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS, CIGAR_EQ = 1, 2, 4, 8, 16, 32
OP_CHARS = " M=XID"


class GapsC(C.Structure):
    _fields_ = [("open", C.c_int8), ("extend", C.c_int8)]


class SizeRangeC(C.Structure):
    _fields_ = [("min", C.c_size_t), ("max", C.c_size_t)]


class RectangleC(C.Structure):
    _fields_ = [("row", C.c_size_t), ("col", C.c_size_t), ("width", C.c_size_t), ("height", C.c_size_t)]


class AlignResultC(C.Structure):
    _fields_ = [("score", C.c_int32), ("query_idx", C.c_size_t), ("reference_idx", C.c_size_t)]


class OpLenC(C.Structure):
    _fields_ = [("op", C.c_uint8), ("len", C.c_size_t)]


class AlignStatsC(C.Structure):
    """struct BaAlignStats (include/block_aligner_hip.h): the per-alignment statistics of the ba_*_stats calls."""
    _fields_ = [("q_start", C.c_uint32), ("r_start", C.c_uint32), ("columns", C.c_uint32), ("matches", C.c_uint32),
                ("mismatches", C.c_uint32), ("positives", C.c_uint32), ("ins", C.c_uint32), ("del", C.c_uint32),
                ("gap_opens", C.c_uint32), ("longest_ins", C.c_uint32), ("longest_del", C.c_uint32), ("path_score", C.c_int32)]


STATS_DTYPE = np.dtype(AlignStatsC)
if C.sizeof(AlignStatsC) != 48 or STATS_DTYPE.itemsize != 48:
    raise ImportError(f"struct BaAlignStats must be 48 bytes, the binding declares {C.sizeof(AlignStatsC)}")


TEXT_CIGAR, TEXT_MD, TEXT_CS, TEXT_SOFT_CLIP = 0, 1, 2, 1 << 8   # ba_*_text: the format, and the CIGAR's soft-clip flag
STATS_FAILED_BITS = 1 | 2 | 4 | 8 | 16 | 32 | 128   # status bits (overflow, lost, watchdog) after which a record is all zeros and a text empty


class ExactC(C.Structure):
    """struct BaExact (include/block_aligner_hip.h): one record of the ba_*_exact calls."""
    _fields_ = [("score", C.c_int32), ("query_idx", C.c_uint32), ("reference_idx", C.c_uint32), ("rows", C.c_uint32)]


class ExactPathC(C.Structure):
    """struct BaExactPath: one record of the ba_*_exact_paths calls."""
    _fields_ = [("score", C.c_int32), ("q_start", C.c_uint32), ("r_start", C.c_uint32), ("q_end", C.c_uint32), ("r_end", C.c_uint32),
                ("rows", C.c_uint32)]


class ChainingParamsC(C.Structure):
    """struct BaChainingParams (include/block_aligner_hip.h): the parameters of the ba_chaining_* calls."""
    _fields_ = [("match_w", C.c_int32), ("drift_cost", C.c_int32), ("skip_cost", C.c_int32), ("lookback", C.c_uint32), ("max_dist", C.c_uint32),
                ("bandwidth", C.c_uint32), ("max_chains", C.c_uint32), ("min_score", C.c_int32), ("min_anchors", C.c_uint32)]


class SeedingParamsC(C.Structure):
    """struct BaSeedingParams (include/block_aligner_hip.h): the parameters of the ba_seeding_* calls."""
    _fields_ = [("k", C.c_uint32), ("w", C.c_uint32), ("max_occ", C.c_uint32)]


class SelectParamsC(C.Structure):
    """struct BaSelectParams (include/block_aligner_hip.h): the parameters of the ba_select_* calls."""
    _fields_ = [("mask_permille", C.c_uint32), ("sec_permille", C.c_uint32), ("max_secondary", C.c_uint32), ("mapq_max", C.c_uint32),
                ("full_support", C.c_uint32), ("min_score", C.c_int32)]


SEL_PRIMARY, SEL_SUPPLEMENTARY, SEL_SECONDARY, SEL_DROPPED, SEL_EXCLUDED = 0, 1, 2, 3, 4   # Selector.results()["cls"]
SEL_NONE = 0xffffffff                                                                         # parent and rank of an excluded candidate


class AccuracyC(C.Structure):
    """struct BaAccuracy: what ba_accuracy_summary reports."""
    _fields_ = [("n", C.c_uint64), ("compared", C.c_uint64), ("skipped", C.c_uint64), ("wrong", C.c_uint64), ("below", C.c_uint64),
                ("above", C.c_uint64), ("diff_end", C.c_uint64), ("mean_rel_error", C.c_double), ("min_diff", C.c_int32), ("max_diff", C.c_int32)]


EXACT_DTYPE = np.dtype(ExactC)
if C.sizeof(ExactC) != 16 or EXACT_DTYPE.itemsize != 16:
    raise ImportError(f"struct BaExact must be 16 bytes, the binding declares {C.sizeof(ExactC)}")
EXACT_PATH_DTYPE = np.dtype(ExactPathC)
if C.sizeof(ExactPathC) != 24 or EXACT_PATH_DTYPE.itemsize != 24:
    raise ImportError(f"struct BaExactPath must be 24 bytes, the binding declares {C.sizeof(ExactPathC)}")
EXACT_GLOBAL, EXACT_EXTEND = 0, 1   # ba_*_exact: the quantity
EXACT_OWN_MODE = 1 << 8             # ... and the flag bit: under the batch's own start / end rules, or its profile's gap costs
EXACT_TRACE_MAX_CELLS = 1 << 31     # ba_*_exact_cigars: |q| * |r| of a pair


def _text_list(buf, off):
    s = buf.tobytes().decode("ascii")
    o = off.tolist()
    return [s[o[p]:o[p + 1]] for p in range(len(o) - 1)]


@dataclass(frozen=True)
class AlignResult:
    score: int
    query_idx: int
    reference_idx: int


# The same kernels behind a host side that reads the BA_* development switches (environment variables): for the tests that force
# a code path on small inputs and for the measurement scripts under tools/. The release library reads no environment variables.
DEV_LIB_PATH = os.path.join(_HERE, "lib", "libblock_aligner_hip_dev.so")
_lib = None
_loaded = {}


def use_library(path: str) -> None:
    """Route every later call through another build of the library (objects must not outlive the switch)."""
    global LIB_PATH, _lib
    LIB_PATH = path
    _lib = _loaded.get(path)


def lib() -> C.CDLL:
    """Load the HIP library; raises if it has not been built (python -c 'import __graft_entry__ as g; g.build()')."""
    global _lib
    if _lib is None and LIB_PATH in _loaded:
        _lib = _loaded[LIB_PATH]
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                               "block_aligner_amd has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, sz, u32, i32, i8, u8p = C.c_void_p, C.c_size_t, C.c_uint32, C.c_int32, C.c_int8, C.c_char_p
        L.ba_last_error.restype = C.c_char_p
        L.ba_host_alloc.restype = vp
        L.ba_host_alloc.argtypes = [C.c_uint64]
        L.ba_host_free.argtypes = [vp]
        L.ba_set_device.argtypes = [C.c_int]
        L.block_percent_len.restype = sz
        L.block_percent_len.argtypes = [sz, C.c_float]
        for k in ("aa", "nuc", "bytes"):
            getattr(L, f"block_new_padded_{k}").restype = vp
            getattr(L, f"block_new_padded_{k}").argtypes = [sz, sz]
            getattr(L, f"block_set_bytes_padded_{k}").argtypes = [vp, u8p, sz, sz]
            getattr(L, f"block_free_padded_{k}").argtypes = [vp]
        for k in ("aa", "nuc"):
            getattr(L, f"block_set_bytes_rev_padded_{k}").argtypes = [vp, u8p, sz, sz]
        L.block_new_cigar.restype = vp
        L.block_new_cigar.argtypes = [sz, sz]
        L.block_get_cigar.restype = OpLenC
        L.block_get_cigar.argtypes = [vp, sz]
        L.block_len_cigar.restype = sz
        L.block_len_cigar.argtypes = [vp]
        L.block_free_cigar.argtypes = [vp]
        L.block_new_generic.restype = vp
        L.block_new_generic.argtypes = [u32, sz, sz, sz]
        L.block_align_generic.argtypes = [vp, C.c_int, vp, vp, vp, GapsC, SizeRangeC, i32]
        L.block_res_generic.restype = AlignResultC
        L.block_res_generic.argtypes = [vp]
        L.block_cigar_generic.argtypes = [vp, sz, sz, vp]
        L.block_cigar_eq_generic.argtypes = [vp, vp, vp, sz, sz, vp]
        L.block_free_generic.argtypes = [vp]
        L.block_align_profile_generic.argtypes = [vp, vp, vp, SizeRangeC, i32]
        L.block_trace_blocks_generic.restype = sz
        L.block_trace_blocks_generic.argtypes = [vp, vp, sz]
        L.block_batch_align_exp.argtypes = [C.c_int, vp, GapsC, SizeRangeC, i32, i32, u32, vp, vp, vp, vp, vp, sz, vp, vp]
        L.block_batch_align_profile_exp.argtypes = [vp, SizeRangeC, i32, i32, u32, vp, vp, vp, sz, vp, vp]
        L.block_new_aaprofile.restype = vp
        L.block_new_aaprofile.argtypes = [sz, sz, i8]
        L.block_free_aaprofile.argtypes = [vp]
        L.ba_aaprofile_set_raw.argtypes = [vp, vp, vp, vp, vp, sz]
        L.ba_batch_create_profile.restype = vp
        L.ba_batch_create_profile.argtypes = [vp, SizeRangeC, i32, u32, vp, vp, vp, sz]
        L.ba_batch_create.restype = vp
        L.ba_batch_create.argtypes = [C.c_int, vp, GapsC, SizeRangeC, i32, u32, vp, vp, vp, vp, vp, sz]
        L.ba_batch_reload.argtypes = [vp, vp, vp, vp, vp, vp, sz]
        L.ba_batch_reload_profile.argtypes = [vp, vp, vp, vp, vp, sz]
        L.ba_batch_launch.argtypes = [vp]
        L.ba_batch_wait.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_set_wait_limit_ms.argtypes = [C.c_uint64]; L.ba_set_wait_limit_ms.restype = None
        L.ba_batch_compact_cigars.argtypes = [vp, vp, C.c_uint64]
        L.ba_batch_surviving_cells.argtypes = [vp, vp]
        L.ba_batch_retried.argtypes = [vp]
        L.ba_device_memory.argtypes = [vp, vp]
        L.ba_batch_info.argtypes = [vp, vp]
        L.ba_batch_kernel.argtypes = [vp]
        L.ba_batch_geometry.argtypes = [vp]
        L.ba_batch_spec_cells.argtypes = [vp, vp]
        L.ba_batch_skipped_cells.argtypes = [vp, vp]
        L.ba_build_id.restype = C.c_char_p
        L.ba_multibatch_create.restype = vp
        L.ba_multibatch_create.argtypes = [C.c_int, vp, GapsC, SizeRangeC, i32, u32, vp, vp, vp, vp, vp, sz, vp, C.c_int]
        L.ba_multibatch_parts.argtypes = [vp, vp, C.c_int]
        L.ba_sized_batch_create.restype = vp
        L.ba_sized_batch_create.argtypes = [C.c_int, vp, GapsC, vp, i32, u32, vp, vp, vp, vp, vp, sz]
        L.ba_sized_batch_create_percent.restype = vp
        L.ba_sized_batch_create_percent.argtypes = [C.c_int, vp, GapsC, C.c_float, C.c_float, i32, u32, vp, vp, vp, vp, vp, sz]
        L.ba_sized_batch_classes.argtypes = [vp, vp, vp, vp, vp, C.c_int]
        L.ba_multibatch_kernel_ms.argtypes = [vp, vp, C.c_int]
        L.ba_shard_slices.argtypes = [vp, vp, sz, C.c_int, vp]
        L.ba_extend_batch_create.restype = vp
        L.ba_extend_batch_create.argtypes = [C.c_int, vp, GapsC, SizeRangeC, i32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]
        L.ba_extend_batch_reload.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]
        L.ba_extend_batch_times.argtypes = [vp, vp, vp, vp]
        L.ba_chain_batch_create.restype = vp
        L.ba_chain_batch_create.argtypes = [C.c_int, vp, GapsC, SizeRangeC, i32, u32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]
        L.ba_chain_batch_reload.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz]
        L.ba_chain_batch_times.argtypes = [vp, vp, vp, vp, vp]
        L.ba_chain_batch_run.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_chain_batch_results.argtypes = [vp] * 11
        L.ba_chain_batch_cigars.argtypes = [vp, vp, C.c_uint64]
        L.ba_chain_batch_destroy.argtypes = [vp]
        L.ba_chaining_create.restype = vp
        L.ba_chaining_create.argtypes = [C.POINTER(ChainingParamsC), vp, vp, vp, vp, sz]
        L.ba_chaining_reload.argtypes = [vp, vp, vp, vp, vp, sz]
        L.ba_chaining_run.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_chaining_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
        L.ba_chaining_results.argtypes = [vp] * 9
        L.ba_chaining_dp.argtypes = [vp, vp, vp]
        L.ba_chaining_times.argtypes = [vp, vp, vp, vp]
        L.ba_chaining_destroy.argtypes = [vp]
        L.ba_chaining_create_seeded.restype = vp
        L.ba_chaining_create_seeded.argtypes = [C.POINTER(ChainingParamsC), vp]
        L.ba_select_create.restype = vp
        L.ba_select_create.argtypes = [C.POINTER(SelectParamsC)] + [vp] * 8 + [sz, sz]
        L.ba_select_create_chained.restype = vp
        L.ba_select_create_chained.argtypes = [C.POINTER(SelectParamsC), vp, vp, vp, sz]
        L.ba_select_reload.argtypes = [vp] * 9 + [sz, sz]
        L.ba_select_run.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_select_counts.argtypes = [vp, C.POINTER(C.c_uint64), vp]
        L.ba_select_results.argtypes = [vp] * 6
        L.ba_select_kept.argtypes = [vp, vp, vp]
        L.ba_select_times.argtypes = [vp, vp, vp, vp]
        L.ba_select_destroy.argtypes = [vp]
        L.ba_seeding_create.restype = vp
        L.ba_seeding_create.argtypes = [C.POINTER(SeedingParamsC), vp, vp, vp, vp, vp, vp, sz]
        L.ba_seeding_reload.argtypes = [vp, vp, vp, vp, vp, vp, vp, sz]
        L.ba_seeding_run.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_seeding_counts.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), vp]
        L.ba_seeding_results.argtypes = [vp] * 5
        L.ba_seeding_sketch.argtypes = [vp] * 7
        L.ba_seeding_times.argtypes = [vp, vp, vp, vp]
        L.ba_seeding_destroy.argtypes = [vp]
        L.ba_ref_index_create.restype = vp
        L.ba_ref_index_create.argtypes = [u32, u32, vp, C.c_uint64]
        L.ba_ref_index_counts.argtypes = [vp] * 6
        L.ba_ref_index_entries.argtypes = [vp] * 3
        L.ba_ref_index_times.argtypes = [vp] * 4
        L.ba_ref_index_destroy.argtypes = [vp]
        L.ba_seeding_create_indexed.restype = vp
        L.ba_seeding_create_indexed.argtypes = [vp, u32, u32, vp, vp, vp, vp, sz]
        L.ba_seeding_reload_indexed.argtypes = [vp, vp, vp, vp, vp, sz]
        L.ba_chain_windows.argtypes = [vp] * 7 + [sz, u32, vp, vp, vp]
        L.ba_ref_index_create_multi.restype = vp
        L.ba_ref_index_create_multi.argtypes = [u32, u32, vp, vp, vp, sz]
        L.ba_ref_index_sequences.argtypes = [vp, C.POINTER(C.c_uint64), vp]
        L.ba_ref_index_create_canonical.restype = vp
        L.ba_ref_index_create_canonical.argtypes = [u32, u32, vp, vp, vp, sz]
        L.ba_ref_index_is_canonical.argtypes = [vp, C.POINTER(C.c_int)]
        L.ba_seeding_create_indexed_both.restype = vp
        L.ba_seeding_create_indexed_both.argtypes = [vp, u32, u32, vp, vp, vp, sz]
        L.ba_seeding_reload_indexed_both.argtypes = [vp, vp, vp, vp, sz]
        L.ba_seeding_problems.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        L.ba_chaining_create_bounded.restype = vp
        L.ba_chaining_create_bounded.argtypes = [C.POINTER(ChainingParamsC), vp, vp, vp, vp, sz, vp, sz]
        L.ba_chain_windows_seqs.argtypes = [vp] * 5 + [sz, u32, vp, vp, sz] + [vp] * 5
        L.ba_ref_locate.argtypes = [vp, sz, vp, vp, sz, vp, vp, vp, vp]
        for f, fields in (("ba_batch", 6), ("ba_sized_batch", 6), ("ba_multibatch", 6), ("ba_extend_batch", 10)):   # the calls of _Batch
            getattr(L, f"{f}_run").argtypes = [vp, C.POINTER(C.c_float)]
            getattr(L, f"{f}_results").argtypes = [vp] * (1 + fields)
            getattr(L, f"{f}_cigars").argtypes = [vp, vp, C.c_uint64]
            getattr(L, f"{f}_stats").argtypes = [vp, vp]
            getattr(L, f"{f}_text").argtypes = [vp, C.c_uint32, vp, vp, C.c_uint64]
            getattr(L, f"{f}_destroy").argtypes = [vp]
        L.ba_chain_batch_stats.argtypes = [vp, vp]
        L.ba_chain_batch_text.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint64]
        L.ba_chain_batch_report_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float)]
        for f in ("ba_batch", "ba_sized_batch", "ba_multibatch"):
            getattr(L, f"{f}_exact").argtypes = [vp, u32, i32, vp, sz, vp]
            getattr(L, f"{f}_exact_cigars").argtypes = [vp, u32, i32, vp, sz, vp, vp, vp, C.c_uint64]
            getattr(L, f"{f}_exact_paths").argtypes = [vp, u32, i32, vp, sz, vp, vp, vp, sz]
        L.ba_extend_batch_exact.argtypes = [vp, i32, vp, sz, vp, vp, vp]
        L.ba_extend_batch_exact_paths.argtypes = [vp, i32, vp, sz, vp, vp, vp, vp, vp, sz]
        L.ba_batch_exact_paths_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        L.ba_exact_paths_check_lengths_profile.argtypes = [vp, vp, sz]
        L.ba_batch_exact_cigars_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        L.ba_exact_trace_check_lengths.argtypes = [vp, vp, sz]
        L.ba_batch_exact_ms.argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_uint64)]
        L.ba_exact_check_lengths.argtypes = [vp, vp, sz]
        L.ba_exact_check_lengths_profile.argtypes = [vp, vp, sz]
        L.ba_accuracy_summary.argtypes = [vp, vp, vp, vp, vp, sz, C.POINTER(AccuracyC)]
        L.ba_batch_stats_ms.argtypes = [vp, C.POINTER(C.c_float)]
        L.ba_batch_text_ms.argtypes = [vp, C.POINTER(C.c_float)]
        _lib = L
        _loaded[LIB_PATH] = L
    return _lib


_pinned = {}   # base address -> (bytes, owning library) of the live ba_host_alloc buffers


def pinned_array(n: int, dtype=np.uint32) -> np.ndarray:
    """A numpy array over page-locked host memory (ba_host_alloc): pass it as `out=` to BatchAligner.compact_cigars / cigars. Free it with
    free_pinned(array) when done (nothing else frees it); arrays from anywhere else are refused where the device writes through them."""
    nbytes = int(n) * np.dtype(dtype).itemsize
    p = lib().ba_host_alloc(nbytes)
    if not p:
        raise RuntimeError(last_error())
    _pinned[p] = (nbytes, lib())
    return np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p)).view(dtype)


def is_pinned(a: np.ndarray) -> bool:
    """True if `a` lies inside a live pinned_array() buffer."""
    addr = a.ctypes.data
    return any(base <= addr and addr + a.nbytes <= base + nb for base, (nb, _) in _pinned.items())


def free_pinned(a: np.ndarray) -> None:
    """ba_host_free for an array made by pinned_array (the array must not be used afterwards)."""
    ent = _pinned.pop(a.ctypes.data, None)
    if ent is None:
        raise ValueError("not the start of a pinned_array() buffer")
    ent[1].ba_host_free(a.ctypes.data)


def last_error() -> str:
    return lib().ba_last_error().decode()


def device_count() -> int:
    return lib().ba_device_count()


def set_device(d: int) -> None:
    if lib().ba_set_device(d):
        raise RuntimeError(last_error())


def device_memory():
    """(free, total) bytes of the selected device."""
    f, t = C.c_uint64(), C.c_uint64()
    if lib().ba_device_memory(C.byref(f), C.byref(t)):
        raise RuntimeError(last_error())
    return f.value, t.value


def percent_len(length: int, p: float) -> int:
    """lib.rs:109-111"""
    return lib().block_percent_len(length, p)


def _kind_name(matrix_cls) -> str:
    return {0: "aa", 1: "nuc", 2: "bytes"}[matrix_cls.KIND]


def _size(size) -> SizeRangeC:
    if isinstance(size, range):  # Rust `a..=b` written as range(a, b + 1)
        return SizeRangeC(size.start, size.stop - 1)
    return SizeRangeC(int(size[0]), int(size[1]))


def _gaps(gaps) -> GapsC:
    return GapsC(gaps.open, gaps.extend) if isinstance(gaps, S.Gaps) else GapsC(gaps[0], gaps[1])


def accuracy_summary(score, exact, query_idx=None, reference_idx=None, status=None) -> dict:
    """ba_accuracy_summary (needs no device): the results of a run (score[, query_idx, reference_idx, status]) against exact records of the
    same pairs -- `exact` is an EXACT_DTYPE array, a dict of arrays as _Batch.exact() returns, or plain exact scores. -> dict: n, compared,
    skipped (failure status), wrong (exact != score), below (score < exact), above, diff_end, mean_rel_error (mean of (exact - score) / |exact|
    over the wrong pairs with exact != 0), min_diff, max_diff (of exact - score over the wrong pairs; 0 if none)."""
    score = np.ascontiguousarray(score, dtype=np.int32)
    n = len(score)
    if isinstance(exact, dict):
        rec = np.zeros(n, EXACT_DTYPE)
        for k in EXACT_DTYPE.names:
            rec[k] = exact[k]
    elif getattr(exact, "dtype", None) == EXACT_DTYPE:
        rec = np.ascontiguousarray(exact)
    else:
        rec = np.zeros(n, EXACT_DTYPE)
        rec["score"] = exact
    opt = [None if a is None else np.ascontiguousarray(a, dtype=np.uint32) for a in (query_idx, reference_idx, status)]
    if len(rec) != n or any(a is not None and len(a) != n for a in opt):
        raise ValueError("score, exact, query_idx, reference_idx and status must have one entry per pair")
    out = AccuracyC()
    if lib().ba_accuracy_summary(score.ctypes.data, *_ptrs(opt), rec.ctypes.data, n, C.byref(out)):
        raise RuntimeError(last_error())
    return {k: getattr(out, k) for k, _ in AccuracyC._fields_}


def exact_trace_check_lengths(q_len, r_len) -> None:
    """The length guards of exact_cigars() on their own (needs no device): exact_check_lengths' and |q| * |r| <= EXACT_TRACE_MAX_CELLS."""
    q_len, r_len = np.ascontiguousarray(q_len, np.uint32), np.ascontiguousarray(r_len, np.uint32)
    if len(q_len) != len(r_len):
        raise ValueError("q_len and r_len must have one entry per pair")
    if lib().ba_exact_trace_check_lengths(q_len.ctypes.data, r_len.ctypes.data, len(q_len)):
        raise RuntimeError(last_error())


def exact_paths_check_lengths_profile(q_len, r_len) -> None:
    """The length guards of exact_paths() on a profile batch on their own (needs no device; r_len: profile lengths):
    exact_check_lengths_profile's and (|q| + 1) * |r| <= EXACT_TRACE_MAX_CELLS."""
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32)
    r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    if lib().ba_exact_paths_check_lengths_profile(q_len.ctypes.data, r_len.ctypes.data, len(q_len)):
        raise RuntimeError(last_error())


def exact_check_lengths_profile(q_len, r_len) -> None:
    """The length guard of exact(own_mode=True) on a profile batch on its own (needs no device; r_len: profile lengths): raises, naming the
    pair, if (|q| + |r|) * 384 -- three int8 terms per column -- does not stay above the sentinel -2^30."""
    q_len, r_len = np.ascontiguousarray(q_len, dtype=np.uint32), np.ascontiguousarray(r_len, dtype=np.uint32)
    if len(q_len) != len(r_len):
        raise ValueError("q_len and r_len must have one entry per pair")
    if lib().ba_exact_check_lengths_profile(q_len.ctypes.data, r_len.ctypes.data, len(q_len)):
        raise RuntimeError(last_error())


def exact_check_lengths(q_len, r_len) -> None:
    """The length guard of the exact calls on its own (needs no device): raises, naming the pair, if one is too long for int32 scores."""
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32); r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    if lib().ba_exact_check_lengths(q_len.ctypes.data, r_len.ctypes.data, len(q_len)):
        raise RuntimeError(last_error())


def _which(which):
    """-> (array or None, address, count) of a pair selection."""
    if which is None:
        return None, None, 0
    w = np.ascontiguousarray(which, dtype=np.uint32)
    return w, w.ctypes.data, len(w)


def _pair_arrays(pool, q_off, q_len, *r):
    """pool, q_off, q_len[, r_off, r_len] as the C calls take them: contiguous uint8 bytes, uint64 offsets, uint32 lengths."""
    return [np.ascontiguousarray(a, dtype=t) for a, t in zip((pool, q_off, q_len) + r, (np.uint8, np.uint64, np.uint32, np.uint64, np.uint32))]


def _ptrs(arrays):
    """The arrays' addresses (None stays None); keep the arrays referenced until the call has returned."""
    return [a.ctypes.data if a is not None else None for a in arrays]


class PaddedBytes:
    """scan_block.rs:1790-1884. `matrix_cls` plays the role of the `<M: Matrix>` type parameter."""

    def __init__(self, length: int, block_size: int, matrix_cls=S.AAMatrix):
        self.kind = matrix_cls.KIND
        self._k = _kind_name(matrix_cls)
        self._h = getattr(lib(), f"block_new_padded_{self._k}")(length, block_size)
        self._len = length
        self._cap = length

    new = classmethod(lambda cls, length, block_size, matrix_cls=S.AAMatrix: cls(length, block_size, matrix_cls))

    @classmethod
    def from_bytes(cls, b: bytes, block_size: int, matrix_cls=S.AAMatrix) -> "PaddedBytes":
        p = cls(len(b), block_size, matrix_cls)
        p.set_bytes(b, block_size)
        return p

    from_str = classmethod(lambda cls, s, block_size, matrix_cls=S.AAMatrix: cls.from_bytes(s.encode(), block_size, matrix_cls))

    def set_bytes(self, b: bytes, block_size: int) -> None:
        getattr(lib(), f"block_set_bytes_padded_{self._k}")(self._h, bytes(b), len(b), block_size)
        self._len = len(b)

    def set_bytes_rev(self, b: bytes, block_size: int) -> None:
        getattr(lib(), f"block_set_bytes_rev_padded_{self._k}")(self._h, bytes(b), len(b), block_size)
        self._len = len(b)

    def len(self) -> int:
        return self._len

    __len__ = len

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            getattr(_lib, f"block_free_padded_{self._k}")(self._h)
            self._h = None


class Cigar:
    """cigar.rs:42-163"""

    def __init__(self, query_len: int, reference_len: int):
        self._h = lib().block_new_cigar(query_len, reference_len)

    new = classmethod(lambda cls, q, r: cls(q, r))

    def len(self) -> int:
        return lib().block_len_cigar(self._h)

    __len__ = len

    def get(self, i: int):
        o = lib().block_get_cigar(self._h, i)
        return (o.op, o.len)

    def to_vec(self):
        return [self.get(i) for i in range(self.len())]

    def __str__(self) -> str:
        return "".join(f"{n}{OP_CHARS[op]}" for op, n in self.to_vec() if op)

    to_string = __str__

    def format(self, q: bytes, r: bytes):
        a, b, i, j = [], [], 0, 0
        for op, n in self.to_vec():
            for _ in range(n):
                if op in (1, 2, 3):
                    a.append(chr(q[i])); b.append(chr(r[j])); i += 1; j += 1
                elif op == 4:
                    a.append(chr(q[i])); b.append("-"); i += 1
                elif op == 5:
                    a.append("-"); b.append(chr(r[j])); j += 1
        return "".join(a), "".join(b)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.block_free_cigar(self._h)
            self._h = None


class _NativeProfile:
    """The library's AAProfile object (ffi.rs:60-195) filled from the numpy mirror in scores.AAProfile."""

    def __init__(self, p: S.AAProfile):
        L = lib()
        self._h = L.block_new_aaprofile(p.str_len, p.curr_len - p.str_len - 1, p.gap_extend)
        pos = np.ascontiguousarray(p.pos_aa[: p.curr_len], dtype=np.int8)
        g = [np.ascontiguousarray(a[: p.curr_len], dtype=np.int8) for a in (p.pos_gap_open_C, p.pos_gap_close_C, p.pos_gap_open_R)]
        if L.ba_aaprofile_set_raw(self._h, pos.ctypes.data, g[0].ctypes.data, g[1].ctypes.data, g[2].ctypes.data, p.curr_len):
            raise RuntimeError(last_error())

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.block_free_aaprofile(self._h)
            self._h = None


class _Trace:
    def __init__(self, block: "Block"):
        self._b = block

    def cigar(self, i: int, j: int, cigar: Cigar) -> None:
        lib().block_cigar_generic(self._b._h, i, j, cigar._h)

    def cigar_eq(self, q: PaddedBytes, r: PaddedBytes, i: int, j: int, cigar: Cigar) -> None:
        lib().block_cigar_eq_generic(self._b._h, q._h, r._h, i, j, cigar._h)

    def blocks(self):
        """Trace::blocks() (scan_block.rs:1676-1691): [(row, col, width, height), ...] in fill order."""
        n = lib().block_trace_blocks_generic(self._b._h, None, 0)
        arr = (RectangleC * max(n, 1))()
        lib().block_trace_blocks_generic(self._b._h, arr, n)
        return [(r.row, r.col, r.width, r.height) for r in arr[:n]]


class Block:
    """Block::<TRACE, X_DROP, LOCAL_START, FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS> (scan_block.rs:89, 798-1244)."""

    def __init__(self, query_len: int, reference_len: int, max_size: int, trace: bool = False, x_drop: bool = False,
                 local_start: bool = False, free_query_start_gaps: bool = False, free_query_end_gaps: bool = False):
        self.mode = (TRACE * trace) | (X_DROP * x_drop) | (LOCAL_START * local_start) | \
                    (FREE_QUERY_START_GAPS * free_query_start_gaps) | (FREE_QUERY_END_GAPS * free_query_end_gaps)
        self._h = lib().block_new_generic(self.mode, query_len, reference_len, max_size)

    new = classmethod(lambda cls, *a, **k: cls(*a, **k))

    def align(self, query: PaddedBytes, reference: PaddedBytes, matrix, gaps, size, x_drop: int = 0) -> None:
        raw = matrix.raw()
        lib().block_align_generic(self._h, matrix.KIND, query._h, reference._h, raw.ctypes.data, _gaps(gaps), _size(size), x_drop)

    def align_exp(self, query, reference, matrix, gaps, size, x_drop: int, target_score: int):
        """scan_block.rs:884-902: double the min block size until the score reaches the target."""
        s = _size(size)
        mn, mx = max(s.min, 16), max(s.max, 16)
        while mn <= mx:
            self.align(query, reference, matrix, gaps, (mn, mx), x_drop)
            if self.res().score >= target_score:
                return mn
            mn *= 2
        return None

    def align_profile(self, query: PaddedBytes, profile: S.AAProfile, size, x_drop: int = 0) -> None:
        """scan_block.rs:942-968"""
        native = _NativeProfile(profile)
        lib().block_align_profile_generic(self._h, query._h, native._h, _size(size), x_drop)

    def align_profile_exp(self, query, profile, size, x_drop: int, target_score: int):
        """scan_block.rs:974-992"""
        s = _size(size)
        mn, mx = max(s.min, 16), max(s.max, 16)
        while mn <= mx:
            self.align_profile(query, profile, (mn, mx), x_drop)
            if self.res().score >= target_score:
                return mn
            mn *= 2
        return None

    def res(self) -> AlignResult:
        r = lib().block_res_generic(self._h)
        return AlignResult(r.score, r.query_idx, r.reference_idx)

    def trace(self) -> _Trace:
        assert self.mode & TRACE, "Block was created without TRACE"
        return _Trace(self)

    def __del__(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.block_free_generic(self._h)
            self._h = None


class _Batch:
    """What the four batch aligners share: run, results, cigars, stats, text and close over the C calls `<_C>_run`, `_results`, `_cigars`,
    `_stats`, `_text` and `_destroy`. A subclass sets _C and, if its results have other fields, RESULTS; its constructor sets n, mode and _h."""

    _C = ""
    RESULTS = (("score", np.int32), ("query_idx", np.uint32), ("reference_idx", np.uint32), ("cells", np.uint64), ("cigar_len", np.uint32),
               ("status", np.uint32))

    def _call(self, name, *args):
        if getattr(lib(), f"{self._C}_{name}")(self._h, *args):
            raise RuntimeError(last_error())

    def run(self) -> float:
        """Launch and wait; returns the kernel's HIP-event time in milliseconds."""
        ms = C.c_float()
        self._call("run", C.byref(ms))
        return ms.value

    def results(self):
        out = {k: np.zeros(self.n, t) for k, t in self.RESULTS}
        self._call("results", *_ptrs(out.values()))
        return out

    def cigars(self, cigar_len=None):
        """-> (runs, offsets): runs[offsets[p]:offsets[p+1]] are pair p's packed (len << 4 | op) runs."""
        return self._cigars(cigar_len)

    def _cigars(self, cigar_len, out=None):
        if cigar_len is None:
            cigar_len = self.results()["cigar_len"]
        off = np.zeros(self.n + 1, np.uint64)
        np.cumsum(cigar_len, out=off[1:])
        total = int(off[-1])
        runs = out[:total] if out is not None and out.size >= total else np.empty(total, np.uint32)
        self._call("cigars", runs.ctypes.data, runs.size)
        return runs, off

    def stats(self):
        """TRACE batches after a run: per-alignment statistics in pair order (ba_*_stats) -> dict of arrays: q_start, r_start, columns,
        matches, mismatches, positives, ins, del, gap_opens, longest_ins, longest_del, path_score, plus identity = matches / columns (0 where
        columns == 0) and edit_distance = mismatches + ins + del (SAM NM)."""
        rec = np.zeros(self.n, STATS_DTYPE)
        self._call("stats", rec.ctypes.data)
        out = {k: rec[k].copy() for k in STATS_DTYPE.names}
        cols = out["columns"]
        out["identity"] = np.divide(out["matches"], cols, out=np.zeros(self.n, np.float64), where=cols > 0)
        out["edit_distance"] = out["mismatches"] + out["ins"] + out["del"]
        return out

    def exact(self, what=None, x_drop=-1, which=None, own_mode=False):
        """Exact full-matrix scores of the batch's pairs, computed on the device (ba_*_exact; no run needed) -> dict of arrays score,
        query_idx, reference_idx, rows. what: EXACT_GLOBAL (H[|q|][|r|]) or EXACT_EXTEND (the maximum over the matrix; with x_drop >= 0
        under the row-wise X-drop rule); None = EXACT_EXTEND for an X-drop batch, EXACT_GLOBAL otherwise. which: pair indices in any order,
        repeats allowed (record k belongs to which[k]); None = every pair. own_mode (EXACT_OWN_MODE in what): the matrix of the batch's own
        mode -- LOCAL_START / FREE_QUERY_* start and end rules, a profile's position-specific gap costs --, which is refused without it;
        on a plain sequence batch it changes nothing."""
        if what is None:
            what = EXACT_EXTEND if self.mode & X_DROP else EXACT_GLOBAL
        if own_mode:
            what = int(what) | EXACT_OWN_MODE
        w, wp, wn = _which(which)
        rec = np.zeros(self.n if w is None else wn, EXACT_DTYPE)
        self._call("exact", int(what), int(x_drop), wp, wn, rec.ctypes.data)
        return {k: rec[k].copy() for k in EXACT_DTYPE.names}

    def exact_cigars(self, what=None, x_drop=-1, which=None):
        """The optimal alignment paths of the exact full-matrix DP, computed on the device (ba_*_exact_cigars; no run needed) -> (records as
        exact(), runs, off): runs[off[k]:off[k + 1]] are record k's packed (len << 4 | op) runs, in the format of cigars(); '=' / 'X' in a
        CIGAR_EQ batch, 'M' otherwise. what, x_drop and which as in exact()."""
        if what is None:
            what = EXACT_EXTEND if self.mode & X_DROP else EXACT_GLOBAL
        w, wp, wn = _which(which)
        m = self.n if w is None else wn
        rec, off = np.zeros(m, EXACT_DTYPE), np.zeros(m + 1, np.uint64)   # the two-call pattern: records and offsets, then the runs
        self._call("exact_cigars", int(what), int(x_drop), wp, wn, rec.ctypes.data, off.ctypes.data, None, 0)
        runs = np.zeros(int(off[-1]), np.uint32)
        self._call("exact_cigars", int(what), int(x_drop), wp, wn, rec.ctypes.data, off.ctypes.data, runs.ctypes.data, runs.size)
        return {k: rec[k].copy() for k in EXACT_DTYPE.names}, runs, off

    def exact_paths(self, what=None, x_drop=-1, which=None):
        """The optimal alignment paths in the batch's own mode, computed on the device (ba_*_exact_paths; no run needed) -> (rec, runs,
        off). Every batch is served: LOCAL_START / FREE_QUERY_* batches, profile batches, plain ones (where the runs are exact_cigars()'s).
        rec: dict of arrays score, q_start, r_start, q_end, r_end, rows -- score, (q_end, r_end) and rows are exact(own_mode=True)'s score,
        end cell and rows, (q_start, r_start) is the cell where the backward walk stopped. runs[off[k]:off[k + 1]] are record k's packed
        (len << 4 | op) runs over q[q_start:q_end] and r[r_start:r_end]; '=' / 'X' in a CIGAR_EQ sequence batch, 'M' otherwise. what,
        x_drop and which as in exact(); EXACT_OWN_MODE in what changes nothing."""
        if what is None:
            what = EXACT_EXTEND if self.mode & X_DROP else EXACT_GLOBAL
        w, wp, wn = _which(which)
        m = self.n if w is None else wn
        rec, off = np.zeros(m, EXACT_PATH_DTYPE), np.zeros(m + 1, np.uint64)   # the two-call pattern: records and offsets, then the runs
        self._call("exact_paths", int(what), int(x_drop), wp, wn, rec.ctypes.data, off.ctypes.data, None, 0)
        runs = np.zeros(int(off[-1]), np.uint32)
        self._call("exact_paths", int(what), int(x_drop), wp, wn, rec.ctypes.data, off.ctypes.data, runs.ctypes.data, runs.size)
        return {k: rec[k].copy() for k in EXACT_PATH_DTYPE.names}, runs, off

    def accuracy(self, x_drop=-1, which=None, own_mode=False):
        """After a run: the batch's results against exact() of the same pairs (accuracy_summary) -> dict. own_mode as in exact()."""
        ex = self.exact(None, x_drop, which, own_mode)
        res = self.results()
        sel = slice(None) if which is None else np.asarray(which, dtype=np.int64)
        return accuracy_summary(res["score"][sel], ex, res["query_idx"][sel], res["reference_idx"][sel], res["status"][sel])

    def text(self, what=TEXT_CIGAR, soft_clip=False):
        """TRACE batches after a run: every pair's CIGAR (TEXT_CIGAR, with soft_clip its S runs), SAM MD:Z value (TEXT_MD) or short cs:Z value
        (TEXT_CS), rendered on the device (ba_*_text) -> (buf: uint8 array, offsets: uint64 array of n + 1); pair p's text is
        buf[offsets[p]:offsets[p + 1]], empty for a pair without runs or with a failure status."""
        w = int(what) | (TEXT_SOFT_CLIP if soft_clip else 0)
        off = np.zeros(self.n + 1, np.uint64)   # the two-call pattern: sizes, then text
        self._call("text", w, off.ctypes.data, None, 0)
        buf = np.zeros(int(off[-1]), np.uint8)
        if buf.size:
            self._call("text", w, off.ctypes.data, buf.ctypes.data, buf.size)
        return buf, off

    def text_list(self, what=TEXT_CIGAR, soft_clip=False):
        """text() as one str per pair."""
        return _text_list(*self.text(what, soft_clip))

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            getattr(_lib, f"{self._C}_destroy")(self._h)
            self._h = None

    __del__ = close


class BatchAligner(_Batch):
    """Batch launcher: many independent pairs, one persistent kernel launch, one wavefront per pair.

    pool: uint8 array of raw sequence bytes; pair p = pool[q_off[p]:+q_len[p]] (query) vs pool[r_off[p]:+r_len[p]].
    """

    _C = "ba_batch"

    def __init__(self, matrix, gaps, size, x_drop: int, mode: int, pool, q_off, q_len, r_off, r_len):
        self.n = len(q_len)
        self.mode = mode
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len)
        raw = matrix.raw()
        self._h = lib().ba_batch_create(matrix.KIND, raw.ctypes.data, _gaps(gaps), _size(size), x_drop, mode, *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())

    def reload(self, pool, q_off, q_len, r_off, r_len) -> None:
        """Replace the pairs and keep the device buffers (ba_batch_reload): the new set must fit the original one's sizes."""
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len)
        self._call("reload", *_ptrs(a), len(a[2]))
        self.n = len(a[2])

    def launch(self) -> None:
        """Enqueue one pass on the batch's stream and return (ba_batch_launch); wait() collects it."""
        self._call("launch")

    def compact_cigars(self, pinned_out=None) -> None:
        """Between launch() and wait(): gather the CIGAR runs on the device behind the kernels -- straight into `pinned_out` (an array
        from pinned_array(); pass the same array as cigars(out=...)) or into a device buffer (cigars() is then one copy)."""
        if pinned_out is not None and not is_pinned(pinned_out):
            raise ValueError("compact_cigars writes through this buffer from the device: it must come from pinned_array()")
        self._call("compact_cigars", pinned_out.ctypes.data if pinned_out is not None else None, pinned_out.size if pinned_out is not None else 0)

    def wait(self) -> float:
        ms = C.c_float()
        self._call("wait", C.byref(ms))
        return ms.value

    def cigars(self, cigar_len=None, out=None):
        """-> (runs, offsets): runs[offsets[p]:offsets[p+1]] are pair p's packed (len << 4 | op) runs. out: a uint32 array to reuse
        (a fresh 600 MB array costs more in page faults than the copy into it)."""
        return self._cigars(cigar_len, out)

    def surviving_cells(self):
        """TRACE batches: per pair, sum of width x height over Trace::blocks() (scan_block.rs:1676-1691)."""
        out = np.zeros(self.n, np.uint64)
        self._call("surviving_cells", out.ctypes.data)
        return out

    def retried(self) -> int:
        """Pairs the last run re-ran with full-size trace slots (ba_batch_retried)."""
        return lib().ba_batch_retried(self._h)

    def stats_ms(self) -> float:
        """HIP-event time of the last stats() kernel in milliseconds."""
        ms = C.c_float()
        self._call("stats_ms", C.byref(ms))
        return ms.value

    def exact_ms(self):
        """(HIP-event milliseconds, cells) of the last exact() call: cells = the sum of rows * (|r| + 1) over the request."""
        ms, cells = C.c_float(), C.c_uint64()
        self._call("exact_ms", C.byref(ms), C.byref(cells))
        return ms.value, int(cells.value)

    def exact_cigars_ms(self):
        """(HIP-event milliseconds, cells) of the last exact_cigars() call that computed: sweep, walk, offsets and gather."""
        ms, cells = C.c_float(), C.c_uint64()
        self._call("exact_cigars_ms", C.byref(ms), C.byref(cells))
        return ms.value, int(cells.value)

    def exact_paths_ms(self):
        """(HIP-event milliseconds, cells) of the last exact_paths() call that computed: sweep, walk, offsets and gather."""
        ms, cells = C.c_float(), C.c_uint64()
        self._call("exact_paths_ms", C.byref(ms), C.byref(cells))
        return ms.value, int(cells.value)

    def text_ms(self) -> float:
        """HIP-event time of the text kernels the last text() call ran (the sizes, then the rendering), in milliseconds."""
        ms = C.c_float()
        self._call("text_ms", C.byref(ms))
        return ms.value

    KERNELS = ("k_align", "k_multi", "k_quad", "k_small")

    def spec_cells(self) -> int:
        """Cells of the last run's speculative, untraced rectangles (X-drop + TRACE): a part of results()["cells"]."""
        o = C.c_uint64()
        self._call("spec_cells", C.byref(o))
        return int(o.value)

    def skipped_cells(self) -> int:
        """Cells of the last run that were not computed: padding columns of the blocks that close X-drop alignments. Counted in results()["cells"]."""
        o = C.c_uint64()
        self._call("skipped_cells", C.byref(o))
        return int(o.value)

    def info(self):
        o = np.zeros(4, np.uint64)
        lib().ba_batch_info(self._h, o.ctypes.data)
        return dict(grid=int(o[0]), lds_bytes_per_wave=int(o[1]), trace_arena_bytes=int(o[2]), pool_bytes=int(o[3]),
                    kernel=self.KERNELS[lib().ba_batch_kernel(self._h)], geometry=lib().ba_batch_geometry(self._h))


def shard_slices(q_len, r_len, parts: int) -> np.ndarray:
    """ba_shard_slices: boundaries of `parts` contiguous slices of near-equal summed |q| + |r| (needs no device)."""
    q_len = np.ascontiguousarray(q_len, dtype=np.uint32); r_len = np.ascontiguousarray(r_len, dtype=np.uint32)
    bounds = np.zeros(parts + 1, np.uint64)
    if lib().ba_shard_slices(q_len.ctypes.data, r_len.ctypes.data, len(q_len), parts, bounds.ctypes.data):
        raise RuntimeError(last_error())
    return bounds


class MultiBatchAligner(_Batch):
    """One batch over several GPUs (ba_multibatch_*): contiguous cost-balanced slices, one per entry of `devices`."""

    _C = "ba_multibatch"

    def __init__(self, matrix, gaps, size, x_drop: int, mode: int, pool, q_off, q_len, r_off, r_len, devices):
        self.n = len(q_len)
        self.mode = mode
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len)
        raw = matrix.raw()
        dev = np.ascontiguousarray(devices, dtype=np.int32)
        self._h = lib().ba_multibatch_create(matrix.KIND, raw.ctypes.data, _gaps(gaps), _size(size), x_drop, mode, *_ptrs(a), self.n,
                                             dev.ctypes.data, len(dev))
        if not self._h:
            raise RuntimeError(last_error())

    def kernel_ms(self):
        """Kernel time of every slice in the last run() (ms; HIP events on the slice's own stream)."""
        t = np.zeros(64, np.float32)
        k = lib().ba_multibatch_kernel_ms(self._h, t.ctypes.data, 64)
        if k < 0:   # (the last run did not complete)
            raise RuntimeError(last_error())
        return t[:k].copy()

    def parts(self):
        b = np.zeros(65, np.uint64)
        k = lib().ba_multibatch_parts(self._h, b.ctypes.data, 65)
        return b[: k + 1].copy()


class SizedBatchAligner(_Batch):
    """Every pair with its own block range (ba_sized_batch_*): `sizes` = an (n, 2) array of (min, max), or percent = (min_percent, max_percent) of
    the longer sequence's length per pair, as examples/nanopore_bench_global.rs:144-171 calls percent_len."""

    _C = "ba_sized_batch"

    def __init__(self, matrix, gaps, x_drop: int, mode: int, pool, q_off, q_len, r_off, r_len, sizes=None, percent=None):
        L = lib()
        self.n = len(q_len)
        self.mode = mode
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len)
        raw = matrix.raw()
        if (sizes is None) == (percent is None):
            raise ValueError("give either sizes or percent")
        if sizes is not None:
            sz = np.ascontiguousarray(sizes, dtype=np.uint64).reshape(self.n, 2)   # SizeRange {uintptr min, max}
            self._h = L.ba_sized_batch_create(matrix.KIND, raw.ctypes.data, _gaps(gaps), sz.ctypes.data, x_drop, mode, *_ptrs(a), self.n)
        else:
            self._h = L.ba_sized_batch_create_percent(matrix.KIND, raw.ctypes.data, _gaps(gaps), percent[0], percent[1], x_drop, mode, *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())

    def classes(self):
        """[(min, max, pairs, fill kernel, kernel ms of the last run)] per bin."""
        cap = 64
        while True:   # (the call returns the number of bins, however many fit: a second call with room for all of them if there are more)
            r = np.zeros((cap, 2), np.uint64); c = np.zeros(cap, np.uint64); k = np.zeros(cap, np.int32); t = np.zeros(cap, np.float32)
            nb = lib().ba_sized_batch_classes(self._h, r.ctypes.data, c.ctypes.data, k.ctypes.data, t.ctypes.data, cap)
            if nb < 0:   # (the last run did not complete)
                raise RuntimeError(last_error())
            if nb <= cap:
                break
            cap = nb
        return [(int(r[i, 0]), int(r[i, 1]), int(c[i]), int(k[i]), float(t[i])) for i in range(nb)]


class ProfileBatchAligner(BatchAligner):
    """Sequence-to-profile batch: pair p aligns the amino-acid query pool[q_off[p]:+q_len[p]] to profiles[p]
    (Block::align_profile over many pairs, examples/pssm_bench.rs:86-103)."""

    def __init__(self, profiles, size, x_drop: int, mode: int, pool, q_off, q_len):
        self.n = len(q_len)
        self.mode = mode
        a = _pair_arrays(pool, q_off, q_len)
        natives = [_NativeProfile(p) for p in profiles]
        arr = (C.c_void_p * self.n)(*[x._h for x in natives])
        self._h = lib().ba_batch_create_profile(arr, _size(size), x_drop, mode, *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())


class ExtendBatchAligner(_Batch):
    """Seed-and-extend batch (ba_extend_batch_*): per seed p, X-drop extension leftwards from q[q_seed[p]] / r[r_seed[p]] (reversed prefixes)
    and rightwards from the seed's end, spliced with the seed into one result. q = pool[q_off[p]:+q_len[p]], r = pool[r_off[p]:+r_len[p]];
    strand (NucMatrix only; None = all 0): 1 aligns the reverse complement of q, and the seed coordinates and results are in that frame.
    mode must hold X_DROP; TRACE and CIGAR_EQ are optional. Arguments are checked before the device is touched.

    run() fills both sides of every seed, then splices, and returns the fill kernel's time. cigars() gives seed p's runs; stats() and text()
    describe the spliced path from (q_start, r_start) over the oriented query (the reverse complement on the minus strand), text()'s soft
    clips are against the whole query."""

    _C = "ba_extend_batch"
    RESULTS = (("score", np.int32), ("q_start", np.uint32), ("r_start", np.uint32), ("q_end", np.uint32), ("r_end", np.uint32),
               ("left_score", np.int32), ("right_score", np.int32), ("cells", np.uint64), ("cigar_len", np.uint32), ("status", np.uint32))

    @staticmethod
    def _arrays(pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand):
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len) + [np.ascontiguousarray(x, dtype=np.uint32) for x in (q_seed, r_seed, seed_len)] + \
            [None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)]
        n = len(a[2])
        if any(len(x) != n for x in a[1:] if x is not None):
            raise ValueError("q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len and strand must have one entry per seed")
        return a

    def __init__(self, matrix, gaps, size, x_drop: int, mode: int, pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand=None):
        a = self._arrays(pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand)
        self.n = len(a[2])
        self.mode = mode
        raw = matrix.raw()
        self._h = lib().ba_extend_batch_create(matrix.KIND, raw.ctypes.data, _gaps(gaps), _size(size), x_drop, mode, *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())

    def reload(self, pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand=None) -> None:
        """Replace the seeds and keep the device buffers (ba_extend_batch_reload): the new set must fit the original one's sizes."""
        a = self._arrays(pool, q_off, q_len, r_off, r_len, q_seed, r_seed, seed_len, strand)
        self._call("reload", *_ptrs(a), len(a[2]))
        self.n = len(a[2])

    @property
    def exact_cigars(self):
        raise AttributeError("extension batches have no exact_cigars (exact paths are out of scope for them: INTEGRATION.md)")

    def exact(self, x_drop=-1, which=None, own_mode=False):
        """EXACT_EXTEND on both sides of every seed (ba_extend_batch_exact; no run needed) -> dict: left and right (dicts of arrays score,
        query_idx, reference_idx, rows; an empty side is all zeros) and score = left + the seed's ungapped score + right. own_mode is
        refused: ba_extend_batch_exact has no `what`, and an extension batch is created without the modes the flag is for."""
        if own_mode:
            raise RuntimeError("exact: EXACT_OWN_MODE does not apply to extension batches (they are created without LOCAL_START / "
                               "FREE_QUERY_* and without profiles; ba_extend_batch_exact takes no `what`)")
        w, wp, wn = _which(which)
        m = self.n if w is None else wn
        left, right, score = np.zeros(m, EXACT_DTYPE), np.zeros(m, EXACT_DTYPE), np.zeros(m, np.int32)
        self._call("exact", int(x_drop), wp, wn, left.ctypes.data, right.ctypes.data, score.ctypes.data)
        return dict(left={k: left[k].copy() for k in EXACT_DTYPE.names}, right={k: right[k].copy() for k in EXACT_DTYPE.names}, score=score)

    def exact_paths(self, what=None, x_drop=-1, which=None):
        """The optimal path of every seed's extension (ba_extend_batch_exact_paths; no run needed) -> (rec, runs, off): the left side's
        EXACT_EXTEND path turned round + the seed's ungapped columns + the right side's path, merged. rec: score (left + seed + right),
        q_start, r_start, q_end, r_end (the coordinates of results()), rows (left + right), and the sides' records as exact() gives them
        in the dicts left / right. what: None or EXACT_EXTEND (extension batches have no other quantity)."""
        if what is not None and int(what) & ~EXACT_OWN_MODE != EXACT_EXTEND:
            raise RuntimeError("exact: an extension batch has one quantity, EXACT_EXTEND on both sides of the seed")
        w, wp, wn = _which(which)
        m = self.n if w is None else wn
        rec, off = np.zeros(m, EXACT_PATH_DTYPE), np.zeros(m + 1, np.uint64)
        left, right = np.zeros(m, EXACT_DTYPE), np.zeros(m, EXACT_DTYPE)
        self._call("exact_paths", int(x_drop), wp, wn, rec.ctypes.data, left.ctypes.data, right.ctypes.data, off.ctypes.data, None, 0)
        runs = np.zeros(int(off[-1]), np.uint32)
        self._call("exact_paths", int(x_drop), wp, wn, rec.ctypes.data, left.ctypes.data, right.ctypes.data, off.ctypes.data, runs.ctypes.data, runs.size)
        out = {k: rec[k].copy() for k in EXACT_PATH_DTYPE.names}
        out["left"] = {k: left[k].copy() for k in EXACT_DTYPE.names}
        out["right"] = {k: right[k].copy() for k in EXACT_DTYPE.names}
        return out, runs, off

    def accuracy(self, x_drop=-1, which=None):
        """After a run: the spliced scores against exact()'s (accuracy_summary without the end comparison) -> dict."""
        ex = self.exact(x_drop, which)
        res = self.results()
        sel = slice(None) if which is None else np.asarray(which, dtype=np.int64)
        return accuracy_summary(res["score"][sel], ex["score"], status=res["status"][sel])

    def times(self):
        """Device milliseconds: fill and splice of the last run(), image packers of the last create / reload."""
        f, p, s = C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(f), C.byref(p), C.byref(s))
        return dict(fill_ms=f.value, pack_ms=p.value, splice_ms=s.value)


class ChainBatchAligner(_Batch):
    """Anchor-chain batch (ba_chain_batch_*): chain c holds the anchors anchor_first[c] .. anchor_first[c + 1] (anchor_first: one entry per
    chain and one more, from 0), anchor k at q[q_anchor[k]:+anchor_len[k]] / r[r_anchor[k]:+anchor_len[k]] of the chain's sequences
    q = pool[q_off[c]:+q_len[c]], r = pool[r_off[c]:+r_len[c]]. The stretches between consecutive anchors are aligned globally, the two ends
    of the chain extended with X-drop as the sides of a seed, and everything spliced into one result per chain on the device. strand as for
    ExtendBatchAligner. mode must hold X_DROP; TRACE and CIGAR_EQ are optional. Arguments are checked before the device is touched.

    run() fills the ends, then the gaps, then splices, and returns both fills' time. results() has ExtendBatchAligner's keys; cigars() gives
    chain c's runs; report() gives the chains' statistics and CIGAR / MD / cs strings (ChainReport). The exact scores of chain batches are
    not offered ("Anchor chains")."""

    _C = "ba_chain_batch"
    RESULTS = ExtendBatchAligner.RESULTS

    @staticmethod
    def _arrays(pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand):
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len) + [np.ascontiguousarray(anchor_first, dtype=np.uint64)] + \
            [np.ascontiguousarray(x, dtype=np.uint32) for x in (q_anchor, r_anchor, anchor_len)] + \
            [None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)]
        n = len(a[2])
        if any(len(x) != n for x in a[1:5]) or (a[9] is not None and len(a[9]) != n):
            raise ValueError("q_off, q_len, r_off, r_len and strand must have one entry per chain")
        if len(a[5]) != n + 1:
            raise ValueError("anchor_first must have one entry per chain and one more")
        if any(len(x) != len(a[6]) for x in a[7:9]) or (n and len(a[6]) != int(a[5][-1])):
            raise ValueError("q_anchor, r_anchor and anchor_len must have one entry per anchor (anchor_first[-1] of them)")
        return a

    def __init__(self, matrix, gaps, size, x_drop: int, mode: int, pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len,
                 strand=None):
        a = self._arrays(pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand)
        self.n = len(a[2])
        self.mode = mode
        raw = matrix.raw()
        self._h = lib().ba_chain_batch_create(matrix.KIND, raw.ctypes.data, _gaps(gaps), _size(size), x_drop, mode, *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())

    def reload(self, pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand=None) -> None:
        """Replace the chains and keep the device buffers (ba_chain_batch_reload): the new set must fit the original one's sizes."""
        a = self._arrays(pool, q_off, q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, strand)
        self._call("reload", *_ptrs(a), len(a[2]))
        self.n = len(a[2])

    def times(self):
        """Device milliseconds: both fills and the splice of the last run(), image packers of the last create / reload."""
        e, g, p, s = C.c_float(), C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(e), C.byref(g), C.byref(p), C.byref(s))
        return dict(ends_ms=e.value, gaps_ms=g.value, pack_ms=p.value, splice_ms=s.value)

    def _not_offered(self, *args, **kwargs):
        raise RuntimeError("chain batches offer run, results, cigars, reload and times only: statistics, strings, exact scores and the "
                           "accuracy report of chain batches are out of scope (INTEGRATION.md, \"Anchor chains\"); the statistics and the "
                           "strings of the chains are report()'s")

    stats = text = text_list = exact = exact_cigars = exact_paths = accuracy = _not_offered

    def report(self) -> "ChainReport":
        """TRACE batches after a run: the chains' statistics and strings (ba_chain_batch_stats, ba_chain_batch_text) -> ChainReport."""
        return ChainReport(self)


class ChainReport:
    """What describes the alignments of a ChainBatchAligner ("Statistics and strings of a chain"): a view of the batch that
    holds no device memory of its own; every call reads the batch as it is then (after a reload and a run: the new set). Chain c's record
    and text are those of its spliced runs -- cigars() -- over the oriented query and the reference, ending at (q_end, r_end); reference
    positions are in the frame the batch was created with (the window after chain_batch_args(margin=...): add last_window_shift)."""

    def __init__(self, batch: ChainBatchAligner):
        self._b = batch

    @property
    def n(self):
        return self._b.n

    def _call(self, name, *args):
        self._b._call(name, *args)

    def stats(self):
        """-> the dict of BatchAligner.stats(), one entry per chain: q_start / r_start are results()'s, path_score == score."""
        return _Batch.stats(self)

    def text(self, what=TEXT_CIGAR, soft_clip=False):
        """-> (buf, offsets) as BatchAligner.text(); soft_clip clips over the oriented query's full length."""
        return _Batch.text(self, what, soft_clip)

    def text_list(self, what=TEXT_CIGAR, soft_clip=False):
        return _text_list(*self.text(what, soft_clip))

    def ms(self):
        """(stats_ms, text_ms): HIP-event times of the kernels of the last stats() / text() call."""
        s, t = C.c_float(), C.c_float()
        self._call("report_ms", C.byref(s), C.byref(t))
        return s.value, t.value


def paf_columns(results, stats, q_len, strand=None, r_shift=None) -> dict:
    """The numeric PAF columns of a chain batch's alignments, in NumPy (no device): results = ChainBatchAligner.results(), stats =
    report().stats(), q_len = the reads' lengths, strand = the batch's strand array (None: all plus), r_shift = what to add to reference
    positions (AnchorChainer.last_window_shift after chain_batch_args(margin=...); None: nothing). -> dict of arrays, one entry per chain:
    q_start / q_end in the read's own frame (on the minus strand the oriented frame mirrored: q_len - q_end, q_len - q_start), strand (b"+" /
    b"-"), t_start / t_end in the reference's frame, n_match (matches), aln_len (columns), nm (edit distance), as_ (score). A chain whose
    status has a failure bit (an all-zero record, empty text) gets zeros (and its strand)."""
    n = len(results["score"])
    q_len = np.asarray(q_len, dtype=np.int64)
    minus = np.zeros(n, bool) if strand is None else np.asarray(strand).astype(bool)
    shift = np.zeros(n, np.int64) if r_shift is None else np.asarray(r_shift, dtype=np.int64)
    if not (len(q_len) == len(minus) == len(shift) == len(stats["columns"]) == n):
        raise ValueError("results, stats, q_len, strand and r_shift must have one entry per chain")
    qs, qe = np.asarray(stats["q_start"], dtype=np.int64), np.asarray(results["q_end"], dtype=np.int64)
    ok = (np.asarray(results["status"]) & STATS_FAILED_BITS) == 0
    z = np.zeros(n, np.int64)
    return dict(q_start=np.where(ok, np.where(minus, q_len - qe, qs), z), q_end=np.where(ok, np.where(minus, q_len - qs, qe), z),
                strand=np.where(minus, b"-", b"+").astype("S1"),
                t_start=np.where(ok, np.asarray(stats["r_start"], dtype=np.int64) + shift, z),
                t_end=np.where(ok, np.asarray(results["r_end"], dtype=np.int64) + shift, z),
                n_match=np.where(ok, np.asarray(stats["matches"], dtype=np.int64), z),
                aln_len=np.where(ok, np.asarray(stats["columns"], dtype=np.int64), z),
                nm=np.where(ok, np.asarray(stats["mismatches"], dtype=np.int64) + np.asarray(stats["ins"], dtype=np.int64) +
                            np.asarray(stats["del"], dtype=np.int64), z),
                as_=np.where(ok, np.asarray(results["score"], dtype=np.int64), z))


def sam_flags(cls, strand=None) -> np.ndarray:
    """The SAM flag bits a selection decides, per candidate: 16 on the minus strand, 256 for a secondary, 2048 for a supplementary
    alignment (cls = Selector.results()["cls"]; strand None: all plus). Dropped and excluded candidates are not reported at all."""
    cls = np.asarray(cls)
    minus = np.zeros(len(cls), bool) if strand is None else np.asarray(strand).astype(bool)
    if len(minus) != len(cls):
        raise ValueError("cls and strand must have one entry per candidate")
    return (16 * minus + 256 * (cls == SEL_SECONDARY) + 2048 * (cls == SEL_SUPPLEMENTARY)).astype(np.uint16)


def paf_lines(q_names, q_len, t_name, t_len, paf, selection, cigars=None, target=None) -> list:
    """Whole PAF lines of a selection, in Python (no device): q_names and q_len per read, t_name / t_len the one reference, paf = the dict of
    paf_columns (per chain), selection = the dict of Selector.results() over the same chains, cigars = the chains' CIGAR strings
    (ChainReport.text_list()) or None. -> one line per kept chain, reads in order and in rank order within a read: the twelve PAF columns
    with the selector's mapq in the twelfth, then tp:A:P (primary, supplementary) or tp:A:S (secondary), NM:i, AS:i, s2:i (the best score
    under a head; heads only) and cg:Z where cigars are given. With target -- per chain the number of its reference sequence
    (AnchorChainer.last_window_seq) -- t_name and t_len are sequences indexed by it."""
    kept, first = selection["kept"], selection["kept_first"]
    if len(q_names) != len(first) - 1 or len(q_len) != len(first) - 1:
        raise ValueError("q_names and q_len must have one entry per read")
    if target is not None:
        if len(target) != len(paf["q_start"]):
            raise ValueError("target must have one entry per chain")
        if len(t_name) != len(t_len) or (len(target) and int(np.max(target)) >= len(t_name)):
            raise ValueError("t_name and t_len must have one entry per reference sequence")
    name = lambda x: x.decode() if isinstance(x, (bytes, bytearray, np.bytes_)) else str(x)
    lines = []
    for r in range(len(first) - 1):
        for c in kept[int(first[r]):int(first[r + 1])].tolist():
            head = int(selection["cls"][c]) != SEL_SECONDARY
            tn, tl = (t_name, t_len) if target is None else (t_name[int(target[c])], t_len[int(target[c])])
            f = [name(q_names[r]), int(q_len[r]), int(paf["q_start"][c]), int(paf["q_end"][c]), name(paf["strand"][c]), name(tn), int(tl),
                 int(paf["t_start"][c]), int(paf["t_end"][c]), int(paf["n_match"][c]), int(paf["aln_len"][c]), int(selection["mapq"][c]),
                 "tp:A:P" if head else "tp:A:S", f"NM:i:{int(paf['nm'][c])}", f"AS:i:{int(paf['as_'][c])}"]
            if head:
                f.append(f"s2:i:{int(selection['sub_score'][c])}")
            if cigars is not None:
                f.append("cg:Z:" + name(cigars[c]))
            lines.append("\t".join(str(x) for x in f))
    return lines


class Selector:
    """Read-level selection on the device (ba_select_*; the rule: INTEGRATION.md, "Selecting a read's alignments"). Candidate c -- a chain
    before alignment, an alignment after it -- belongs to read[c], scores score[c] and covers [q_start[c], q_end[c]) of the oriented read of
    q_len[c] bases on strand[c] (None: all plus); support[c] (None: full) scales the mapping quality, exclude[c] takes a candidate out.
    Candidates may come in any order; a read holds at most 1024. Arguments are checked before the device is touched.

    run() marks every candidate and returns the kernels' time; results() gives cls (SEL_*), mapq, parent, rank and sub_score per candidate in
    the caller's order, and kept_first / kept / kept_per_read: per read, the candidates to report, the primary first."""

    @staticmethod
    def _arrays(read, score, q_start, q_end, q_len, strand, support, exclude):
        a = [np.ascontiguousarray(read, dtype=np.uint32), np.ascontiguousarray(score, dtype=np.int32)] + \
            [np.ascontiguousarray(x, dtype=np.uint32) for x in (q_start, q_end, q_len)] + \
            [None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8), None if support is None else np.ascontiguousarray(support, dtype=np.uint32),
             None if exclude is None else np.ascontiguousarray(exclude, dtype=np.uint8)]
        if any(x is not None and len(x) != len(a[0]) for x in a):
            raise ValueError("read, score, q_start, q_end, q_len, strand, support and exclude must have one entry per candidate")
        return a

    @staticmethod
    def _reads(read, n_reads):
        return int(n_reads) if n_reads is not None else (int(np.max(read)) + 1 if len(read) else 0)

    def __init__(self, mask_permille: int, sec_permille: int, max_secondary: int, mapq_max: int, full_support: int, min_score: int, read, score, q_start,
                 q_end, q_len, strand=None, support=None, exclude=None, n_reads=None):
        a = self._arrays(read, score, q_start, q_end, q_len, strand, support, exclude)
        self.n, self.n_reads = len(a[0]), self._reads(a[0], n_reads)
        self.params = SelectParamsC(mask_permille, sec_permille, max_secondary, mapq_max, full_support, min_score)
        self._res = None
        self._h = lib().ba_select_create(C.byref(self.params), *_ptrs(a), self.n, self.n_reads)
        if not self._h:
            raise RuntimeError(last_error())

    @classmethod
    def from_chain_batch(cls, mask_permille: int, sec_permille: int, max_secondary: int, mapq_max: int, full_support: int, min_score: int,
                         batch: "ChainBatchAligner", read_of_chain, support=None, n_reads=None):
        """A selector over the alignments of a ChainBatchAligner that has run (ba_select_create_chained): candidate c is chain c, of read
        read_of_chain[c]; scores, spans and statuses go from the batch's buffers to the selector's on the device, q_len and strand are the
        batch's, and a chain with a failed status is excluded. The selector does not depend on the batch afterwards; reload() refuses it."""
        read = np.ascontiguousarray(read_of_chain, dtype=np.uint32)
        sup = None if support is None else np.ascontiguousarray(support, dtype=np.uint32)
        if len(read) != batch.n or (sup is not None and len(sup) != batch.n):
            raise ValueError("read_of_chain and support must have one entry per chain")
        self = cls.__new__(cls)
        self._h = None
        self._res = None
        self.n, self.n_reads = len(read), cls._reads(read, n_reads)
        self.params = SelectParamsC(mask_permille, sec_permille, max_secondary, mapq_max, full_support, min_score)
        h = lib().ba_select_create_chained(C.byref(self.params), getattr(batch, "_h", None), read.ctypes.data, None if sup is None else sup.ctypes.data,
                                           self.n_reads)
        if not h:
            raise RuntimeError(last_error())
        self._h = h
        return self

    @classmethod
    def from_chains(cls, mask_permille: int, sec_permille: int, max_secondary: int, mapq_max: int, full_support: int, min_score: int,
                    chainer: "AnchorChainer", read_of_problem, q_len, strand=None, n_reads=None):
        """A selector over the chains of an AnchorChainer that has run, to prune them before they are aligned (host-side glue over
        results()): score = chain_score, the span runs from the chain's first anchor to the end of its last, support = its anchors;
        read_of_problem, q_len and strand are per problem and expanded by chain_problem. results()["kept"] are then the chains to align."""
        res = chainer.results()
        per = [np.asarray(read_of_problem), np.asarray(q_len)] + ([] if strand is None else [np.asarray(strand)])
        if any(len(x) != chainer.n for x in per):
            raise ValueError("read_of_problem, q_len and strand must have one entry per problem")
        cp, first = res["chain_problem"], res["anchor_first"].astype(np.int64)
        last = first[1:] - 1
        return cls(mask_permille, sec_permille, max_secondary, mapq_max, full_support, min_score, per[0][cp], res["chain_score"],
                   res["q_anchor"][first[:-1]], res["q_anchor"][last] + res["anchor_len"][last], per[1][cp], None if strand is None else per[2][cp],
                   (first[1:] - first[:-1]).astype(np.uint32), None, cls._reads(per[0], n_reads))

    def _call(self, name, *args):
        if getattr(lib(), f"ba_select_{name}")(self._h, *args):
            raise RuntimeError(last_error())

    def reload(self, read, score, q_start, q_end, q_len, strand=None, support=None, exclude=None, n_reads=None) -> None:
        """Replace the candidates and keep parameters and device buffers (ba_select_reload): no more candidates and no more reads than at first."""
        a = self._arrays(read, score, q_start, q_end, q_len, strand, support, exclude)
        nr = self._reads(a[0], n_reads)
        self._res = None
        self._call("reload", *_ptrs(a), len(a[0]), nr)
        self.n, self.n_reads = len(a[0]), nr

    def run(self) -> float:
        ms = C.c_float()
        self._res = None
        self._call("run", C.byref(ms))
        return ms.value

    def results(self):
        """-> dict: per candidate cls, mapq, parent, rank, sub_score; kept_first (one entry per read and one more), kept, kept_per_read."""
        if self._res is None:
            nk = C.c_uint64()
            per = np.zeros(self.n_reads, np.uint32)
            self._call("counts", C.byref(nk), per.ctypes.data)
            out = dict(cls=np.zeros(self.n, np.uint8), mapq=np.zeros(self.n, np.uint8), parent=np.zeros(self.n, np.uint32), rank=np.zeros(self.n, np.uint32),
                       sub_score=np.zeros(self.n, np.int32))
            self._call("results", *_ptrs(out.values()))
            out["kept_first"], out["kept"] = np.zeros(self.n_reads + 1, np.uint64), np.zeros(nk.value, np.uint32)
            self._call("kept", out["kept_first"].ctypes.data, out["kept"].ctypes.data)
            out["kept_per_read"] = per
            self._res = out
        return self._res

    def times(self):
        """Device milliseconds of the last run(): the grouping with its scan, the marking with its scan, the emit."""
        g, m, e = C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(g), C.byref(m), C.byref(e))
        return dict(group_ms=g.value, mark_ms=m.value, emit_ms=e.value)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.ba_select_destroy(self._h)
            self._h = None

    __del__ = close


class AnchorChainer:
    """Colinear anchor chaining on the device (ba_chaining_*; the rule: INTEGRATION.md, "Chaining anchors"). Problem p -- one read against one
    reference on one strand -- holds the raw hits anchor_first[p] .. anchor_first[p + 1] (anchor_first: one entry per problem and one more,
    from 0), hit k at q[q_anchor[k]:+anchor_len[k]] / r[r_anchor[k]:+anchor_len[k]], sorted within the problem by (r_anchor + anchor_len,
    q_anchor + anchor_len). Arguments are checked before the device is touched.

    run() computes the chains and returns the kernels' time; results() gives them in the layout ChainBatchAligner takes, dp() the raw fill.
    ChainBatchAligner(m, gaps, size, x_drop, mode, *ch.chain_batch_args(pool, q_off, q_len, r_off, r_len)) aligns every chain found."""

    @staticmethod
    def _arrays(anchor_first, q_anchor, r_anchor, anchor_len):
        a = [np.ascontiguousarray(anchor_first, dtype=np.uint64)] + [np.ascontiguousarray(x, dtype=np.uint32) for x in (q_anchor, r_anchor, anchor_len)]
        if len(a[0]) < 1:
            raise ValueError("anchor_first must have one entry per problem and one more")
        if any(len(x) != len(a[1]) for x in a[2:]) or len(a[1]) != int(a[0][-1]):
            raise ValueError("q_anchor, r_anchor and anchor_len must have one entry per anchor (anchor_first[-1] of them)")
        return a

    def __init__(self, match_w: int, drift_cost: int, skip_cost: int, lookback: int, max_dist: int, bandwidth: int, max_chains: int, min_score: int,
                 min_anchors: int, anchor_first, q_anchor, r_anchor, anchor_len, seq_start=None):
        """seq_start (one entry per sequence and one more, from 0): the anchors lie in the frame of several reference sequences laid end
        to end, and every chain stays inside one (ba_chaining_create_bounded; INTEGRATION.md, "Several sequences")."""
        a = self._arrays(anchor_first, q_anchor, r_anchor, anchor_len)
        self.n = len(a[0]) - 1
        self.n_anchors = len(a[1])
        self.params = ChainingParamsC(match_w, drift_cost, skip_cost, lookback, max_dist, bandwidth, max_chains, min_score, min_anchors)
        self._res = None
        self.seq_start = None if seq_start is None else np.ascontiguousarray(seq_start, dtype=np.uint64)
        if self.seq_start is None:
            self._h = lib().ba_chaining_create(C.byref(self.params), *_ptrs(a), self.n)
        else:
            if len(self.seq_start) < 1:
                raise ValueError("seq_start must have one entry per sequence and one more")
            self._h = lib().ba_chaining_create_bounded(C.byref(self.params), *_ptrs(a), self.n, self.seq_start.ctypes.data, len(self.seq_start) - 1)
        if not self._h:
            raise RuntimeError(last_error())

    @classmethod
    def from_seeder(cls, match_w: int, drift_cost: int, skip_cost: int, lookback: int, max_dist: int, bandwidth: int, max_chains: int, min_score: int,
                    min_anchors: int, seeder: "Seeder"):
        """A chainer over the hits of a Seeder that has run (ba_chaining_create_seeded): the hits go from the seeder's buffers to the chainer's
        on the device, without a round trip through the host. The chainer is like any other afterwards and does not depend on the seeder.
        Over a seeder of a multi-sequence index (RefIndex.from_sequences) the chainer is bounded by the index's sequences: seq_start."""
        self = cls.__new__(cls)
        self._h = None
        self._res = None
        self.seq_start = getattr(seeder, "seq_start", None)
        self.params = ChainingParamsC(match_w, drift_cost, skip_cost, lookback, max_dist, bandwidth, max_chains, min_score, min_anchors)
        h = lib().ba_chaining_create_seeded(C.byref(self.params), seeder._h)
        if not h:
            raise RuntimeError(last_error())
        self._h = h
        self.n = seeder.n
        self.n_anchors = seeder.n_hits
        return self

    def _call(self, name, *args):
        if getattr(lib(), f"ba_chaining_{name}")(self._h, *args):
            raise RuntimeError(last_error())

    def reload(self, anchor_first, q_anchor, r_anchor, anchor_len) -> None:
        """Replace the problems and keep parameters and device buffers (ba_chaining_reload): no more problems and no more anchors than at first."""
        a = self._arrays(anchor_first, q_anchor, r_anchor, anchor_len)
        self._res = None
        self._call("reload", *_ptrs(a), len(a[0]) - 1)
        self.n, self.n_anchors = len(a[0]) - 1, len(a[1])

    def run(self) -> float:
        ms = C.c_float()
        self._res = None
        self._call("run", C.byref(ms))
        return ms.value

    def results(self):
        """-> dict: per kept chain chain_problem, chain_rank, chain_score and anchor_first (one more entry); per kept anchor, in path order,
        q_anchor, r_anchor, anchor_len (trimmed: disjoint and colinear) and anchor_src (the input anchor, an index within its problem); per
        problem chains_per_problem."""
        if self._res is None:
            nc, na = C.c_uint64(), C.c_uint64()
            per = np.zeros(self.n, np.uint32)
            self._call("counts", C.byref(nc), C.byref(na), per.ctypes.data)
            out = dict(chain_problem=np.zeros(nc.value, np.uint32), chain_rank=np.zeros(nc.value, np.uint32), chain_score=np.zeros(nc.value, np.int32),
                       anchor_first=np.zeros(nc.value + 1, np.uint64), q_anchor=np.zeros(na.value, np.uint32), r_anchor=np.zeros(na.value, np.uint32),
                       anchor_len=np.zeros(na.value, np.uint32), anchor_src=np.zeros(na.value, np.uint32))
            self._call("results", *_ptrs(out.values()))
            out["chains_per_problem"] = per
            self._res = out
        return self._res

    def dp(self):
        """The raw fill per input anchor -> (f, pred): pred is an index within the problem, -1 for none."""
        f, pred = np.zeros(self.n_anchors, np.int32), np.zeros(self.n_anchors, np.int32)
        self._call("dp", f.ctypes.data, pred.ctypes.data)
        return f, pred

    def times(self):
        """Device milliseconds of the last run(): the fill, the pick with its offset scans, the gather."""
        f, p, g = C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(f), C.byref(p), C.byref(g))
        return dict(fill_ms=f.value, pick_ms=p.value, gather_ms=g.value)

    def chain_batch_args(self, pool, q_off, q_len, r_off, r_len, strand=None, margin=None, seq_off=None, seq_len=None):
        """The positional arguments of ChainBatchAligner after `mode` for the chains found: the per-problem arrays q_off, q_len, r_off, r_len
        and strand expanded by chain_problem, and the chains' anchors. With a margin every chain's reference is cut to its candidate window
        (chain_windows): reference positions of the batch's results are then relative to the window, and last_window_shift holds what to add
        to them, per chain. With seq_off and seq_len -- the sequences of a multi-sequence index, in whose frame the anchors are -- r_off and
        r_len are None and a margin is required: the windows are chain_windows_seqs', last_window_shift leads to positions in the chain's
        own sequence, and last_window_seq says which one that is."""
        res = self.results()
        if seq_off is not None or seq_len is not None:
            if seq_off is None or seq_len is None or r_off is not None or r_len is not None or margin is None:
                raise ValueError("with seq_off and seq_len, r_off and r_len must be None and a margin is required")
            per = [np.asarray(x) for x in (q_off, q_len)] + ([] if strand is None else [np.asarray(strand)])
            if any(len(x) != self.n for x in per):
                raise ValueError("q_off, q_len and strand must have one entry per problem")
            cp = res["chain_problem"]
            r_off_w, r_len_w, r_anchor_w, self.last_window_seq, self.last_window_shift = chain_windows_seqs(
                per[1][cp], res["anchor_first"], res["q_anchor"], res["r_anchor"], res["anchor_len"], margin, seq_off, seq_len)
            return (pool, per[0][cp], per[1][cp], r_off_w, r_len_w, res["anchor_first"], res["q_anchor"], r_anchor_w, res["anchor_len"],
                    None if strand is None else per[2][cp])
        per = [np.asarray(x) for x in (q_off, q_len, r_off, r_len)] + ([] if strand is None else [np.asarray(strand)])
        if any(len(x) != self.n for x in per):
            raise ValueError("q_off, q_len, r_off, r_len and strand must have one entry per problem")
        cp = res["chain_problem"]
        st = None if strand is None else per[4][cp]
        if margin is None:
            return (pool, per[0][cp], per[1][cp], per[2][cp], per[3][cp], res["anchor_first"], res["q_anchor"], res["r_anchor"], res["anchor_len"], st)
        r_off_w, r_len_w, r_anchor_w, self.last_window_shift = chain_windows(per[1][cp], per[2][cp], per[3][cp], res["anchor_first"], res["q_anchor"],
                                                                             res["r_anchor"], res["anchor_len"], margin)
        return (pool, per[0][cp], per[1][cp], r_off_w, r_len_w, res["anchor_first"], res["q_anchor"], r_anchor_w, res["anchor_len"], st)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.ba_chaining_destroy(self._h)
            self._h = None

    __del__ = close


def chain_windows(q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len, margin: int):
    """Candidate windows of chains (ba_chain_windows; INTEGRATION.md, "Reference index"): per chain, the stretch of its reference that the
    chain can reach with `margin` bases to spare -> (r_off, r_len, r_anchor, shift): ChainBatchAligner's arguments in place of the ones given,
    and per chain what was cut off in front (add it to the reference positions of the batch's results). Host only."""
    a = [np.ascontiguousarray(x, dtype=t) for x, t in zip((q_len, r_off, r_len, anchor_first, q_anchor, r_anchor, anchor_len),
                                                          (np.uint32, np.uint64, np.uint32, np.uint64, np.uint32, np.uint32, np.uint32))]
    n = len(a[0])
    if len(a[1]) != n or len(a[2]) != n or len(a[3]) != n + 1:
        raise ValueError("q_len, r_off and r_len must have one entry per chain, anchor_first one more")
    if any(len(x) != len(a[4]) for x in a[5:]) or len(a[4]) != int(a[3][-1]):
        raise ValueError("q_anchor, r_anchor and anchor_len must have one entry per anchor (anchor_first[-1] of them)")
    r_off_w, r_len_w, r_anchor_w = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(len(a[4]), np.uint32)
    if lib().ba_chain_windows(*_ptrs(a), n, margin, r_off_w.ctypes.data, r_len_w.ctypes.data, r_anchor_w.ctypes.data):
        raise RuntimeError(last_error())
    return r_off_w, r_len_w, r_anchor_w, r_off_w - a[1]


def chain_windows_seqs(q_len, anchor_first, q_anchor, r_anchor, anchor_len, margin: int, seq_off, seq_len):
    """Candidate windows of chains whose anchors are in the frame of a multi-sequence index (ba_chain_windows_seqs; INTEGRATION.md, "Several
    sequences"): a window stays inside the sequence that holds the chain's first anchor -> (r_off, r_len, r_anchor, seq, shift):
    ChainBatchAligner's arguments (r_off in the pool, through seq_off), per chain its sequence, and what to add to the reference positions
    of the batch's results to get positions in that sequence. Host only."""
    a = [np.ascontiguousarray(x, dtype=t) for x, t in zip((q_len, anchor_first, q_anchor, r_anchor, anchor_len), (np.uint32, np.uint64, np.uint32, np.uint32, np.uint32))]
    so, sl = np.ascontiguousarray(seq_off, dtype=np.uint64), np.ascontiguousarray(seq_len, dtype=np.uint32)
    n = len(a[0])
    if len(a[1]) != n + 1:
        raise ValueError("q_len must have one entry per chain, anchor_first one more")
    if any(len(x) != len(a[2]) for x in a[3:]) or len(a[2]) != int(a[1][-1]):
        raise ValueError("q_anchor, r_anchor and anchor_len must have one entry per anchor (anchor_first[-1] of them)")
    if len(so) != len(sl):
        raise ValueError("seq_off and seq_len must have one entry per sequence")
    r_off_w, r_len_w, r_anchor_w = np.zeros(n, np.uint64), np.zeros(n, np.uint32), np.zeros(len(a[2]), np.uint32)
    seq, shift = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    if lib().ba_chain_windows_seqs(*_ptrs(a), n, margin, *_ptrs([so, sl]), len(sl), *_ptrs([r_off_w, r_len_w, r_anchor_w, seq, shift])):
        raise RuntimeError(last_error())
    return r_off_w, r_len_w, r_anchor_w, seq, shift


def locate(seq_len, r_start, r_end) -> dict:
    """From the frame of a multi-sequence index to its sequences (ba_ref_locate; INTEGRATION.md, "Several sequences"): for the closed
    intervals [r_start, r_end] -> dict: seq (the last non-empty sequence that starts at or before r_start), local_start, local_end
    (positions in it) and crosses (the interval reaches into the next sequence). Host only."""
    sl = np.ascontiguousarray(seq_len, dtype=np.uint32)
    a, b = np.ascontiguousarray(r_start, dtype=np.uint32), np.ascontiguousarray(r_end, dtype=np.uint32)
    if len(a) != len(b):
        raise ValueError("r_start and r_end must have one entry per interval")
    n = len(a)
    out = dict(seq=np.zeros(n, np.uint32), local_start=np.zeros(n, np.uint32), local_end=np.zeros(n, np.uint32), crosses=np.zeros(n, np.uint8))
    if lib().ba_ref_locate(*_ptrs([sl]), len(sl), *_ptrs([a, b]), n, *_ptrs(out.values())):
        raise RuntimeError(last_error())
    return out


class RefIndex:
    """The sketch of one reference, built once on the device (ba_ref_index_*; INTEGRATION.md, "Reference index"): the (w, k)-minimizers of
    `ref` on strand 0 under the rule of "Seeding", sorted by (code, position), with a prefix table. Seeder.indexed(index, ...) seeds reads
    against all of it. Arguments are checked before the device is touched; the bytes are not kept.

    canonical=True makes the index of canonical k-mers (ba_ref_index_create_canonical; INTEGRATION.md, "Both strands at once"), which
    Seeder.indexed_both seeds against, every read once for both strands: entries() then gives pos with the k-mer's strand in bit 31."""

    def __init__(self, k: int, w: int, ref, canonical: bool = False):
        r = np.ascontiguousarray(np.frombuffer(ref, np.uint8) if isinstance(ref, (bytes, bytearray)) else ref, dtype=np.uint8)
        n = len(r)
        if n == 0:   # (an empty array has no address)
            r = np.zeros(1, np.uint8)
        self.canonical = bool(canonical)
        if canonical:   # one sequence of a sequence table: chainers over its seeders' hits are bounded by it
            self._multi = True
            self.seq_off, self.seq_len = np.zeros(1, np.uint64), np.array([n], np.uint32)
            self._h = lib().ba_ref_index_create_canonical(k, w, r.ctypes.data, self.seq_off.ctypes.data, self.seq_len.ctypes.data, 1)
        else:
            self._multi = False
            self._h = lib().ba_ref_index_create(k, w, r.ctypes.data, n)
        if not self._h:
            raise RuntimeError(last_error())

    @classmethod
    def from_sequences(cls, k: int, w: int, pool, seq_off=None, seq_len=None, canonical: bool = False):
        """The index of several reference sequences (ba_ref_index_create_multi; INTEGRATION.md, "Several sequences"): sequence s is
        pool[seq_off[s]:+seq_len[s]], or pool is a list of bytes, which is packed here. The sequences lie end to end in the index's
        frame, sequences() says where; no k-mer and no window holds bytes of two. Seeders made from it give hits in that frame, and
        AnchorChainer.from_seeder on them keeps every chain inside one sequence. canonical: as for RefIndex()."""
        if seq_off is None and seq_len is None:
            seqs = [bytes(s) for s in pool]
            seq_len = np.array([len(s) for s in seqs], np.uint32)
            seq_off = np.cumsum(seq_len, dtype=np.uint64) - seq_len
            pool = np.frombuffer(b"".join(seqs), np.uint8)
        elif seq_off is None or seq_len is None:
            raise ValueError("seq_off and seq_len go together")
        p = np.ascontiguousarray(np.frombuffer(pool, np.uint8) if isinstance(pool, (bytes, bytearray)) else pool, dtype=np.uint8)
        so, sl = np.ascontiguousarray(seq_off, dtype=np.uint64), np.ascontiguousarray(seq_len, dtype=np.uint32)
        if len(so) != len(sl):
            raise ValueError("seq_off and seq_len must have one entry per sequence")
        if len(sl) and int((so + sl)[sl > 0].max(initial=0)) > len(p):
            raise ValueError("a sequence ends beyond the pool")
        if len(p) == 0:   # (an empty array has no address)
            p = np.zeros(1, np.uint8)
        self = cls.__new__(cls)
        self._h = None
        self._multi = True
        self.canonical = bool(canonical)
        create = lib().ba_ref_index_create_canonical if canonical else lib().ba_ref_index_create_multi
        h = create(k, w, p.ctypes.data, so.ctypes.data, sl.ctypes.data, len(sl))
        if not h:
            raise RuntimeError(last_error())
        self._h = h
        self.seq_off, self.seq_len = so, sl
        return self

    def sequences(self) -> np.ndarray:
        """seq_start: where the index's sequences start in its frame, and where the last one ends (one entry more than sequences)."""
        n = C.c_uint64()
        self._call("sequences", C.byref(n), None)
        start = np.zeros(n.value + 1, np.uint64)
        self._call("sequences", C.byref(n), start.ctypes.data)
        return start

    def locate(self, r_start, r_end) -> dict:
        """locate() with this index's sequences."""
        return locate(np.diff(self.sequences()), r_start, r_end)

    def _call(self, name, *args):
        if getattr(lib(), f"ba_ref_index_{name}")(self._h, *args):
            raise RuntimeError(last_error())

    def counts(self):
        """-> dict: n_entries, k, w, ref_len and longest_run (the most entries that share one code)."""
        n, ln, k, w, run = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._call("counts", C.byref(n), C.byref(k), C.byref(w), C.byref(ln), C.byref(run))
        return dict(n_entries=n.value, k=k.value, w=w.value, ref_len=ln.value, longest_run=run.value)

    def entries(self):
        """-> (code, pos): the entries, ascending by (code, pos). Of a canonical index pos holds the k-mer's strand in bit 31."""
        n = self.counts()["n_entries"]
        code, pos = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        self._call("entries", code.ctypes.data, pos.ctypes.data)
        return code, pos

    def times(self):
        """Device milliseconds of the build: the sketch, the sort of the keys, the prefix table."""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(a), C.byref(b), C.byref(c))
        return dict(sketch_ms=a.value, sort_ms=b.value, table_ms=c.value)

    def close(self):
        """(Seeders made from the index keep what they need.)"""
        if getattr(self, "_h", None) and _lib is not None:
            _lib.ba_ref_index_destroy(self._h)
            self._h = None

    __del__ = close


class Seeder:
    """Minimizer seeding on the device (ba_seeding_*; the rule: INTEGRATION.md, "Seeding"). Problem p is the read q = pool[q_off[p]:+q_len[p]]
    against the reference stretch r = pool[r_off[p]:+r_len[p]] on strand[p] (1: q is read as its reverse complement, and query positions are
    in that frame, the chain batch's): the pair layout of ChainBatchAligner. k = 4 .. 16, w = 1 .. 64; a code that more than max_occ of the
    query's selected k-mers have gives no hits. Arguments are checked before the device is touched.

    run() computes sketches and hits and returns the kernels' time; results() gives the hits of every problem, sorted by (r_hit, q_hit), as
    AnchorChainer takes them; AnchorChainer.from_seeder(..., seeder) chains them where they lie. Seeder.indexed(index, ...) is the same for
    many reads against the one reference of a RefIndex, and Seeder.indexed_both(index, ...) takes every read once for both strands."""

    @staticmethod
    def _arrays(pool, q_off, q_len, r_off, r_len, strand):
        a = _pair_arrays(pool, q_off, q_len, r_off, r_len) + [None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)]
        n = len(a[2])
        if any(len(x) != n for x in a[1:] if x is not None):
            raise ValueError("q_off, q_len, r_off, r_len and strand must have one entry per problem")
        return a

    def __init__(self, k: int, w: int, max_occ: int, pool, q_off, q_len, r_off, r_len, strand=None):
        a = self._arrays(pool, q_off, q_len, r_off, r_len, strand)
        self.n = self.n_reads = len(a[2])   # (n_reads: what ba_seeding_problems reports; it differs from n for indexed_both() only)
        self.params = SeedingParamsC(k, w, max_occ)
        self._counts = None
        self._h = lib().ba_seeding_create(C.byref(self.params), *_ptrs(a), self.n)
        if not self._h:
            raise RuntimeError(last_error())

    @staticmethod
    def _arrays_indexed(pool, q_off, q_len, strand):
        a = _pair_arrays(pool, q_off, q_len) + [None if strand is None else np.ascontiguousarray(strand, dtype=np.uint8)]
        if any(len(x) != len(a[2]) for x in a[1:] if x is not None):
            raise ValueError("q_off, q_len and strand must have one entry per problem")
        return a

    @classmethod
    def indexed(cls, index: "RefIndex", max_occ: int, max_ref_occ: int, pool, q_off, q_len, strand=None):
        """A seeder whose problem p is read p on strand[p] against the whole reference of a RefIndex (ba_seeding_create_indexed); k and w
        are the index's. A reference entry whose code occurs more than max_ref_occ times in the reference's sketch gives no hits (0xffffffff:
        no cap, and then the hits equal Seeder's with r the whole reference). Everything but reload() works as on any Seeder; sketch() has
        no reference entries."""
        a = cls._arrays_indexed(pool, q_off, q_len, strand)
        self = cls.__new__(cls)
        self._h = None
        self._counts = None
        self.n = self.n_reads = len(a[2])
        h = lib().ba_seeding_create_indexed(getattr(index, "_h", None), max_occ, max_ref_occ, *_ptrs(a), self.n)
        if not h:
            raise RuntimeError(last_error())
        self._h = h
        c = index.counts()
        self.params = SeedingParamsC(c["k"], c["w"], max_occ)
        self.max_ref_occ = max_ref_occ
        self.seq_start = index.sequences() if getattr(index, "_multi", False) else None   # (what a chainer over the hits is bounded by)
        return self

    @classmethod
    def indexed_both(cls, index: "RefIndex", max_occ: int, max_ref_occ: int, pool, q_off, q_len):
        """A seeder that takes every read once and seeds it on both strands against a canonical RefIndex (ba_seeding_create_indexed_both;
        INTEGRATION.md, "Both strands at once"): read r = pool[q_off[r]:+q_len[r]] on strand s is problem 2 r + s. n is the number of
        problems, n_reads that of the reads, and read and strand are the per-problem arrays that chain_batch_args, Selector.from_chain_batch
        and paf_columns take (q_off[seeder.read], q_len[seeder.read], seeder.strand). A code that more than max_occ of a read's entries or more
        than max_ref_occ of the index's have, both strands together, gives no hits. sketch() is per read, with the strand in bit 31 of q_pos."""
        a = cls._arrays_indexed(pool, q_off, q_len, None)[:3]
        self = cls.__new__(cls)
        self._h = None
        self._counts = None
        self.n_reads = len(a[2])
        h = lib().ba_seeding_create_indexed_both(getattr(index, "_h", None), max_occ, max_ref_occ, *_ptrs(a), self.n_reads)
        if not h:
            raise RuntimeError(last_error())
        self._h = h
        c = index.counts()
        self.params = SeedingParamsC(c["k"], c["w"], max_occ)
        self.max_ref_occ = max_ref_occ
        self.seq_start = index.sequences()   # (what a chainer over the hits is bounded by)
        self._set_reads(self.n_reads)
        return self

    def _set_reads(self, n_reads: int) -> None:
        self.n_reads, self.n = n_reads, 2 * n_reads
        self.read = np.repeat(np.arange(n_reads, dtype=np.uint32), 2)
        self.strand = np.tile(np.array([0, 1], np.uint8), n_reads)

    def reload_indexed_both(self, pool, q_off, q_len) -> None:
        """reload() for a seeder made by indexed_both() (ba_seeding_reload_indexed_both): no more reads and no more bytes than at first."""
        a = self._arrays_indexed(pool, q_off, q_len, None)[:3]
        self._counts = None
        self._call("reload_indexed_both", *_ptrs(a), len(a[2]))
        self._set_reads(len(a[2]))

    def reload_indexed(self, pool, q_off, q_len, strand=None) -> None:
        """reload() for a seeder made by indexed() (ba_seeding_reload_indexed)."""
        a = self._arrays_indexed(pool, q_off, q_len, strand)
        self._counts = None
        self._call("reload_indexed", *_ptrs(a), len(a[2]))
        self.n = self.n_reads = len(a[2])

    def _call(self, name, *args):
        if getattr(lib(), f"ba_seeding_{name}")(self._h, *args):
            raise RuntimeError(last_error())

    def reload(self, pool, q_off, q_len, r_off, r_len, strand=None) -> None:
        """Replace the problems and keep parameters and device buffers (ba_seeding_reload): no more problems and no more bytes than at first."""
        a = self._arrays(pool, q_off, q_len, r_off, r_len, strand)
        self._counts = None
        self._call("reload", *_ptrs(a), len(a[2]))
        self.n = self.n_reads = len(a[2])

    def run(self) -> float:
        ms = C.c_float()
        self._counts = None
        self._call("run", C.byref(ms))
        return ms.value

    def counts(self):
        """After run() -> dict: n_hits, n_q_seeds, n_r_seeds and hits_per_problem."""
        if self._counts is None:
            h, q, r = C.c_uint64(), C.c_uint64(), C.c_uint64()
            per = np.zeros(self.n, np.uint32)
            self._call("counts", C.byref(h), C.byref(q), C.byref(r), per.ctypes.data)
            self._counts = dict(n_hits=h.value, n_q_seeds=q.value, n_r_seeds=r.value, hits_per_problem=per)
        return self._counts

    @property
    def n_hits(self) -> int:
        return self.counts()["n_hits"]

    def results(self):
        """After run() -> (hit_first, q_hit, r_hit, hit_len, hits_per_problem): AnchorChainer's anchor_first, q_anchor, r_anchor and anchor_len."""
        c = self.counts()
        first = np.zeros(self.n + 1, np.uint64)
        q, r, ln = (np.zeros(c["n_hits"], np.uint32) for _ in range(3))
        self._call("results", first.ctypes.data, q.ctypes.data, r.ctypes.data, ln.ctypes.data)
        return first, q, r, ln, c["hits_per_problem"]

    def sketch(self):
        """After run(): the raw sketches in position order -> dict: q_first, q_pos, q_code, r_first, r_pos, r_code (first: one entry per
        problem and one more)."""
        c = self.counts()
        n = self.n_reads   # (a both-strand seeder's sketches are per read; for every other seeder a problem is a read)
        out = dict(q_first=np.zeros(n + 1, np.uint64), q_pos=np.zeros(c["n_q_seeds"], np.uint32), q_code=np.zeros(c["n_q_seeds"], np.uint32),
                   r_first=np.zeros(n + 1, np.uint64), r_pos=np.zeros(c["n_r_seeds"], np.uint32), r_code=np.zeros(c["n_r_seeds"], np.uint32))
        self._call("sketch", *_ptrs(out.values()))
        return out

    def times(self):
        """Device milliseconds of the last run(): the sketch, the sort, the match."""
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._call("times", C.byref(a), C.byref(b), C.byref(c))
        return dict(sketch_ms=a.value, sort_ms=b.value, match_ms=c.value)

    def close(self):
        if getattr(self, "_h", None) and _lib is not None:
            _lib.ba_seeding_destroy(self._h)
            self._h = None

    __del__ = close


def batch_align_exp(matrix, gaps, size, x_drop: int, target_score: int, mode: int, pool, q_off, q_len, r_off, r_len):
    """Block::align_exp over a batch (scan_block.rs:884-902) -> (score, query_idx, reference_idx, reached_min) arrays;
    reached_min[p] = 0 where the reference returns None."""
    n = len(q_len)
    a = _pair_arrays(pool, q_off, q_len, r_off, r_len)
    raw = matrix.raw()
    res = (AlignResultC * n)()
    reached = np.zeros(n, np.uint64)
    if lib().block_batch_align_exp(matrix.KIND, raw.ctypes.data, _gaps(gaps), _size(size), x_drop, target_score, mode, *_ptrs(a), n, res,
                                   reached.ctypes.data):
        raise RuntimeError(last_error())
    return _unpack_results(res, n) + (reached,)


def batch_align_profile_exp(profiles, size, x_drop: int, target_score: int, mode: int, pool, q_off, q_len):
    """Block::align_profile_exp over a batch (scan_block.rs:974-992)."""
    n = len(q_len)
    a = _pair_arrays(pool, q_off, q_len)
    natives = [_NativeProfile(p) for p in profiles]
    arr = (C.c_void_p * n)(*[x._h for x in natives])
    res = (AlignResultC * n)()
    reached = np.zeros(n, np.uint64)
    if lib().block_batch_align_profile_exp(arr, _size(size), x_drop, target_score, mode, *_ptrs(a), n, res, reached.ctypes.data):
        raise RuntimeError(last_error())
    return _unpack_results(res, n) + (reached,)


def _unpack_results(res, n):
    a = np.frombuffer(res, dtype=np.dtype([("score", np.int32), ("_pad", np.int32), ("qi", np.uint64), ("ri", np.uint64)]), count=n)
    return a["score"].copy(), a["qi"].copy(), a["ri"].copy()


def runs_to_string(runs) -> str:
    return "".join(f"{int(x) >> 4}{OP_CHARS[int(x) & 15]}" for x in runs)
