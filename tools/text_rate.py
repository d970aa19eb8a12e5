#!/usr/bin/env python3
"""Alignment-string rate on the GPU: config 3 (10 kbp DNA reads, block 128..1024, X-drop 100), TRACE|X_DROP|CIGAR_EQ.
Per format (CIGAR, soft-clipped CIGAR, MD, cs):
  sizes_kernel_ms   text_ms() of the sizes call (k_text_len + k_text_offsets)
  write_kernel_ms   text_ms() of the text call (k_text_write)
  copy_ms_*         wall time of the text call into a pinned / a pageable host buffer, less its kernel time: the device-to-host copy of
                    the text and the offsets, plus the call's own overhead
  bytes             the total text
The Python reference (tests/text_ref.py, as a caller would render on the host from cigars() and the raw sequences) renders a sample of
pairs; its time is scaled to all pairs and reported as extrapolated. The sample's strings must equal the device's.
usage: text_rate.py [pairs] [runs] [sample]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from block_aligner_amd import hip as H, workloads as W   # noqa: E402
from tests import text_ref as T   # noqa: E402

FORMATS = (("CIGAR", H.TEXT_CIGAR, False), ("CIGAR+S", H.TEXT_CIGAR, True), ("MD", H.TEXT_MD, False), ("cs", H.TEXT_CS, False))


def call(b, what, off, buf):
    if H.lib().ba_batch_text(b._h, what, off.ctypes.data, None if buf is None else buf.ctypes.data, 0 if buf is None else buf.size):
        raise RuntimeError(H.last_error())


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 100000
    runs_timed = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    sample = min(n, int(sys.argv[3]) if len(sys.argv) > 3 else 1000)
    w = W.config3(n, workers=16)
    p = w.pairs
    size, x_drop = (128, 1024), w.x_drop
    mode = H.TRACE | H.X_DROP | H.CIGAR_EQ
    out = dict(pairs=n, size=size, x_drop=x_drop, mode="TRACE|X_DROP|CIGAR_EQ", sample=sample)
    b = H.BatchAligner(w.matrix, w.gaps, size, x_drop, mode, p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
    out["fill_ms"] = b.run()
    res = b.results()
    assert not res["status"].any()
    runs, roff = b.cigars(res["cigar_len"])
    out["runs"] = int(roff[-1])
    rng = np.random.default_rng(1)
    pick = np.sort(rng.choice(n, sample, replace=False))
    off = np.zeros(n + 1, np.uint64)
    for name, what, clip in FORMATS:
        wv = what | (H.TEXT_SOFT_CLIP if clip else 0)
        call(b, wv, off, None)
        total = int(off[-1])
        page = np.zeros(total, np.uint8)
        pin = H.pinned_array(total, np.uint8)
        sizes_ms, write_ms, wall_pin, wall_page = [], [], [], []
        for _ in range(runs_timed):
            call(b, H.TEXT_CIGAR if what != H.TEXT_CIGAR else H.TEXT_MD, off, None)   # (another format in between: the sizes are not kept)
            call(b, wv, off, None)
            sizes_ms.append(b.text_ms())
            for buf, wall in ((pin, wall_pin), (page, wall_page)):
                t0 = time.perf_counter()
                call(b, wv, off, buf)
                wall.append((time.perf_counter() - t0) * 1e3)
                write_ms.append(b.text_ms())
        assert np.array_equal(pin, page)
        # the host reference on the sample: render from the runs and the raw sequences
        t0 = time.perf_counter()
        want = []
        for q in pick.tolist():
            x = runs[int(roff[q]):int(roff[q + 1])]
            qs, rs = T.image_letters(p.query(q)), T.image_letters(p.reference(q))
            cq, cr = T.consumed(x)
            want.append(T.render(what, x, qs, rs, int(res["query_idx"][q]) - cq, int(res["reference_idx"][q]) - cr, clip))
        t_ref = (time.perf_counter() - t0) * 1e3
        agree = all(page[int(off[q]):int(off[q + 1])].tobytes().decode("ascii") == s for q, s in zip(pick.tolist(), want))
        assert agree, name
        wk = float(np.median(write_ms))
        out[name] = dict(sizes_kernel_ms=float(np.median(sizes_ms)), write_kernel_ms=wk, kernels_ms=float(np.median(sizes_ms)) + wk,
                         copy_ms_pinned=float(np.median(wall_pin)) - wk, copy_ms_pageable=float(np.median(wall_page)) - wk,
                         bytes=total, python_ref_sample_ms=t_ref, python_ref_ms_extrapolated_to_all_pairs=t_ref * n / sample, sample_agrees=agree)
        H.free_pinned(pin)
    b.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
