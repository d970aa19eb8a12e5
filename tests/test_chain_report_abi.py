"""Statistics and strings of chain batches without a GPU: the three C calls are declared and exported, null arguments are refused with a
message, k_stats_chain compiles for gfx950 without scratch and lives in ba_stats.hip, the Python surface is report() and nothing else, and
paf_columns gets the frames right."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "block_aligner_amd", "csrc")
CALLS = ("ba_chain_batch_stats", "ba_chain_batch_text", "ba_chain_batch_report_ms")

CALLER = """
#include <stddef.h>
#include "block_aligner_hip.h"
int use(BaChainBatch* b, struct BaAlignStats* out, uint64_t* offsets, char* text, uint64_t capacity) {
    float s = 0.0f, t = 0.0f;
    int rc = ba_chain_batch_stats(b, out);
    rc |= ba_chain_batch_text(b, BA_TEXT_CIGAR | BA_TEXT_SOFT_CLIP, offsets, NULL, 0);
    rc |= ba_chain_batch_text(b, BA_TEXT_CS, offsets, text, capacity);
    rc |= ba_chain_batch_report_ms(b, &s, &t) | ba_chain_batch_report_ms(b, NULL, NULL);
    return rc + (out->path_score < 0) + (s + t > 0.0f);
}
"""


def test_the_calls_are_exported(hip):
    lib = ctypes.CDLL(hip.LIB_PATH)
    assert not [n for n in CALLS if not hasattr(lib, n)]
    if os.path.exists(hip.DEV_LIB_PATH):
        dev = ctypes.CDLL(hip.DEV_LIB_PATH)
        assert not [n for n in CALLS if not hasattr(dev, n)]


def test_the_calls_are_declared(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read(), flags=re.S)
    for n in CALLS:
        assert re.search(rf"\b{n}\s*\(", text), n
    src = tmp_path / "caller.c"
    src.write_text(CALLER)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "caller.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_header_states_the_consequences():
    text = " ".join(open(os.path.join(ROOT, "include", "block_aligner_hip.h")).read().split())
    for phrase in ("q_start / r_start equal those of ba_chain_batch_results", "path_score == score", "matches + mismatches + ins + del == columns",
                   "candidate window"):
        assert phrase in text, phrase


def test_null_arguments_are_refused(hip):
    L = hip.lib()
    out = (hip.AlignStatsC * 2)()
    off = (ctypes.c_uint64 * 3)()
    assert L.ba_chain_batch_stats(None, ctypes.byref(out)) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_stats(None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_text(None, hip.TEXT_CIGAR, ctypes.byref(off), None, 0) != 0 and "null batch" in hip.last_error()
    assert L.ba_chain_batch_report_ms(None, None, None) != 0 and "null batch" in hip.last_error()


def test_null_out_and_offsets_are_refused_before_the_device_is_touched():
    """The refusals are decided from the arguments alone: null batch first, then the null argument, in the words of the extension calls."""
    src = open(os.path.join(CSRC, "ba_host.cpp")).read()
    body = src[src.index("int ba_chain_batch_stats(BaChainBatch* e"):]
    body = body[:body.index("\n}\n")]
    order = [body.index(x) for x in ('fail("null batch")', 'fail("null argument")', "created without BA_TRACE", "has not finished a run (ba_chain_batch_run)",
                                     "hipSetDevice")]
    assert order == sorted(order)
    body = src[src.index("static int spliced_text(Spliced* e"):]
    body = body[:body.index("\n}\n")]
    order = [body.index(x) for x in ('fail("null batch")', 'fail("null argument: offsets")', "text_check(", "has not finished a run", "hipSetDevice")]
    assert order == sorted(order)
    for call in ("ba_extend_batch_text", "ba_chain_batch_text"):   # one function serves both
        body = src[src.index(f"int {call}("):]
        assert "return spliced_text(e," in body[:body.index("\n}\n")]


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_the_statistics_kernels_build_for_gfx950_without_scratch(tmp_path):
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(CSRC, "ba_stats.hip"), "-o", str(tmp_path / "ba_stats.o")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    scratch, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
    for k in ("k_stats", "k_stats_extend", "k_stats_chain"):
        hits = [v for f, v in scratch.items() if re.search(rf"\d{k}N", f)]
        assert hits == [0], (k, scratch)


def test_the_kernel_lives_in_the_statistics_unit():
    kernels = lambda f: re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(k_\w+)\s*\(", open(os.path.join(CSRC, f)).read())   # noqa: E731
    assert sorted(kernels("ba_chain.hip")) == ["k_chain_anchors", "k_chain_gather", "k_chain_results"]
    assert sorted(kernels("ba_stats.hip")) == ["k_stats", "k_stats_chain", "k_stats_extend"]
    launch = open(os.path.join(CSRC, "ba_launch.h")).read()
    assert launch.index("ba_launch_stats_extend(") < launch.index("ba_launch_stats_chain(") < launch.index("ba_launch_stats_extend(") + 400


def test_the_python_surface(hip):
    cls = hip.ChainBatchAligner
    assert callable(cls.report) and list(inspect.signature(cls.report).parameters) == ["self"]
    cb = cls.__new__(cls)
    cb._h = None
    for name in ("stats", "text", "text_list", "exact", "exact_cigars", "exact_paths", "accuracy"):
        with pytest.raises(RuntimeError, match="out of scope"):
            getattr(cb, name)()
    rep = cb.report()
    assert isinstance(rep, hip.ChainReport) and not [k for k, v in vars(rep).items() if v is not cb]   # a view: it holds the batch and nothing else
    for name in ("stats", "text", "text_list", "ms"):
        assert callable(getattr(rep, name))
    assert list(inspect.signature(rep.text).parameters) == ["what", "soft_clip"] == list(inspect.signature(rep.text_list).parameters)


def _res(score, q_end, r_end, status):
    return dict(score=np.array(score, np.int32), q_end=np.array(q_end, np.uint32), r_end=np.array(r_end, np.uint32), status=np.array(status, np.uint32))


def _st(q_start, r_start, columns, matches, mismatches, ins, dele):
    a = lambda x: np.array(x, np.uint32)   # noqa: E731
    return {"q_start": a(q_start), "r_start": a(r_start), "columns": a(columns), "matches": a(matches), "mismatches": a(mismatches), "ins": a(ins),
            "del": a(dele)}


def test_paf_columns(hip):
    # chain 0: plus strand, inside the read; 1: minus strand; 2: a failed chain (zero record); 3: minus strand, the whole read; 4: plus, whole
    q_len = [100, 100, 80, 50, 60]
    strand = [0, 1, 1, 1, 0]
    res = _res([150, 90, 7, 100, 120], [90, 70, 33, 50, 60], [480, 260, 12, 1050, 61], [0, 0, 8, 0, 0])
    st = _st([10, 20, 0, 0, 0], [400, 205, 0, 1000, 0], [83, 56, 0, 50, 62], [75, 48, 0, 50, 58], [4, 1, 0, 0, 1], [1, 1, 0, 0, 1], [3, 6, 0, 0, 2])
    shift = [1000, 0, 5, 7, 0]
    got = hip.paf_columns(res, st, q_len, strand, shift)
    want = dict(q_start=[10, 30, 0, 0, 0], q_end=[90, 80, 0, 50, 60], strand=[b"+", b"-", b"-", b"-", b"+"], t_start=[1400, 205, 0, 1007, 0],
                t_end=[1480, 260, 0, 1057, 61], n_match=[75, 48, 0, 50, 58], aln_len=[83, 56, 0, 50, 62], nm=[8, 8, 0, 0, 4], as_=[150, 90, 0, 100, 120])
    assert list(got) == list(want)
    for k, w in want.items():
        assert got[k].tolist() == w, k
    plain = hip.paf_columns(res, st, q_len)   # no strand, no shift: the oriented frame is the read's
    assert plain["q_start"].tolist() == [10, 20, 0, 0, 0] and plain["q_end"].tolist() == [90, 70, 0, 50, 60]
    assert plain["t_start"].tolist() == [400, 205, 0, 1000, 0] and plain["t_end"].tolist() == [480, 260, 0, 1050, 61]
    assert plain["strand"].tolist() == [b"+"] * 5
    only_shift = hip.paf_columns(res, st, q_len, None, shift)
    assert only_shift["t_start"].tolist() == [1400, 205, 0, 1007, 0] and only_shift["q_start"].tolist() == plain["q_start"].tolist()
    for k in got:   # the interval is never empty or reversed, and lies inside the read
        if k != "strand":
            assert got[k].dtype == np.int64
    assert (got["q_start"] <= got["q_end"]).all() and (got["q_end"] <= np.array(q_len)).all()
    with pytest.raises(ValueError, match="one entry per chain"):
        hip.paf_columns(res, st, q_len[:3])
