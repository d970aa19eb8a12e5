"""Read-level selection without a GPU: the C calls are exported by both libraries and declared, a C99 caller compiles, struct BaSelectParams
is 24 bytes, every argument rejection is reported before the device is touched, the kernels compile for gfx950 without scratch, and
paf_lines / sam_flags give the known answer's records."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import select_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("ba_select_create", "ba_select_create_chained", "ba_select_reload", "ba_select_run", "ba_select_counts", "ba_select_results",
         "ba_select_kept", "ba_select_times", "ba_select_destroy")
CALLER = r"""
#include "block_aligner_hip.h"
typedef char params_are_24_bytes[sizeof(struct BaSelectParams) == 24 ? 1 : -1];
int use(const uint32_t* u, const int32_t* score, const uint8_t* b, BaChainBatch* batch) {
    struct BaSelectParams p = {500, 800, 2, 60, 10, 20};
    BaSelect* s = ba_select_create(&p, u, score, u, u, u, b, u, b, 10, 2);
    BaSelect* t = ba_select_create_chained(&p, batch, u, NULL, 2);
    float ms = 0.0f, g, m, e;
    uint64_t nk, first[3]; uint32_t per[2], parent[10], rank[10], kept[10]; uint8_t cls[10], mapq[10]; int32_t sub[10];
    int rc = ba_select_reload(s, u, score, u, u, u, NULL, NULL, NULL, 10, 2);
    rc |= ba_select_run(s, &ms);
    rc |= ba_select_counts(s, &nk, per);
    rc |= ba_select_results(s, cls, mapq, parent, rank, sub);
    rc |= ba_select_kept(s, first, kept);
    rc |= ba_select_times(s, &g, &m, &e);
    rc |= ba_select_times(s, NULL, NULL, NULL);
    rc |= cls[0] == BA_SEL_PRIMARY || cls[0] == BA_SEL_EXCLUDED;
    ba_select_destroy(s);
    ba_select_destroy(t);
    return rc;
}
"""
GOOD = R.KNOWN_PARAMS


def test_select_symbols_are_exported_by_both_libraries(hip):
    for path in (hip.LIB_PATH, hip.DEV_LIB_PATH):
        lib = ctypes.CDLL(path)
        assert not [n for n in CALLS if not hasattr(lib, n)], path


def test_select_calls_are_declared_and_a_c99_caller_compiles(tmp_path):
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


def test_params_are_six_4_byte_fields(hip):
    assert ctypes.sizeof(hip.SelectParamsC) == 24
    assert [f[0] for f in hip.SelectParamsC._fields_] == list(R.Params._fields)
    assert all(ctypes.sizeof(f[1]) == 4 for f in hip.SelectParamsC._fields_)
    assert (hip.SEL_PRIMARY, hip.SEL_SUPPLEMENTARY, hip.SEL_SECONDARY, hip.SEL_DROPPED, hip.SEL_EXCLUDED) == (0, 1, 2, 3, 4)


def _make(hip, P=GOOD, **over):
    """The known answer's ten candidates of two reads."""
    a = {k: np.array(v) for k, v in R.KNOWN.items()}
    a.update(exclude=None, n_reads=2)
    a.update(over)
    return hip.Selector(*P, a["read"], a["score"], a["q_start"], a["q_end"], a["q_len"], a["strand"], a["support"], a["exclude"], a["n_reads"])


def _no_device(hip):
    try:
        return hip.device_count() < 1
    except Exception:
        return True


def _accepted(hip, P=GOOD, **over):
    if _no_device(hip):
        with pytest.raises(RuntimeError, match="no usable HIP device"):
            _make(hip, P, **over)
    else:
        _make(hip, P, **over).close()


def test_a_valid_set_passes_every_check(hip):
    """The set the rejections below are cut from is itself accepted: without a device it gets as far as the device."""
    _accepted(hip)
    _accepted(hip, strand=None, support=None, exclude=np.zeros(10, np.uint8))


@pytest.mark.parametrize("change, message", [
    (dict(mask_permille=0), "mask_permille must be between 1 and 1000"),
    (dict(mask_permille=1001), "mask_permille must be between 1 and 1000"),
    (dict(sec_permille=1001), "sec_permille must be between 0 and 1000"),
    (dict(mapq_max=256), "mapq_max must be between 0 and 255"),
    (dict(full_support=0), "full_support must be between 1 and 65535"),
    (dict(full_support=65536), "full_support must be between 1 and 65535"),
    (dict(min_score=0), "min_score must be at least 1"),
    (dict(min_score=-5), "min_score must be at least 1"),
])
def test_rejects_parameters_out_of_range(hip, change, message):
    with pytest.raises(RuntimeError, match=message):
        _make(hip, GOOD._replace(**change))


def test_accepts_the_extreme_parameters(hip):
    _accepted(hip, R.Params(1, 0, 0, 0, 1, 1))
    _accepted(hip, R.Params(1000, 1000, 0xffffffff, 255, 65535, 0x7fffffff))


def _changed(key, c, value):
    a = np.array(R.KNOWN[key])
    a[c] = value
    return {key: a}


def test_rejects_a_read_from_n_reads(hip):
    with pytest.raises(RuntimeError, match=r"candidate 7: read 2 is not below n_reads \(2\)"):
        _make(hip, **_changed("read", 7, 2))


def test_rejects_a_span_that_runs_backwards(hip):
    with pytest.raises(RuntimeError, match="candidate 3: q_start 901 lies behind q_end 900"):
        _make(hip, **_changed("q_start", 3, 901))


def test_rejects_a_span_past_the_read(hip):
    with pytest.raises(RuntimeError, match=r"candidate 9: q_end 401 lies behind the end of the read \(q_len 400\)"):
        _make(hip, **_changed("q_end", 9, 401))


def test_rejects_a_strand_of_2(hip):
    with pytest.raises(RuntimeError, match="candidate 5: strand must be 0 or 1"):
        _make(hip, **_changed("strand", 5, 2))


def test_rejects_a_read_of_1025_candidates_and_names_it(hip):
    n = 3 + 1025
    read = np.array([0, 2, 2] + [1] * 1025, np.uint32)
    one = np.ones(n, np.uint32)
    args = dict(read=read, score=np.full(n, 50, np.int32), q_start=0 * one, q_end=one, q_len=one, strand=None, support=None, n_reads=3)
    with pytest.raises(RuntimeError, match="read 1 holds more than 1024 candidates"):
        _make(hip, **args)
    for k in ("read", "score", "q_start", "q_end", "q_len"):   # 1024 of them are accepted
        args[k] = args[k][:-1]
    _accepted(hip, **args)


def test_rejects_empty_sets_and_mismatched_arrays(hip):
    z = np.zeros(0, np.uint32)
    with pytest.raises(RuntimeError, match="a selection must hold between 1 and 2\\^28 candidates"):
        hip.Selector(*GOOD, z, z, z, z, z, n_reads=1)
    with pytest.raises(RuntimeError, match="a selection must hold between 1 and 2\\^28 reads"):
        _make(hip, n_reads=0)
    with pytest.raises(ValueError, match="one entry per candidate"):
        _make(hip, score=np.array([1, 2, 3]))
    with pytest.raises(ValueError, match="one entry per candidate"):
        _make(hip, exclude=np.zeros(3, np.uint8))


def test_null_handles_and_null_arguments_are_refused(hip):
    L = hip.lib()
    ms = ctypes.c_float()
    assert L.ba_select_run(None, ctypes.byref(ms)) != 0 and "null batch" in hip.last_error()
    assert L.ba_select_counts(None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_select_results(None, *([None] * 5)) != 0 and "null batch" in hip.last_error()
    assert L.ba_select_kept(None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_select_times(None, None, None, None) != 0 and "null batch" in hip.last_error()
    assert L.ba_select_reload(None, *([None] * 8), 0, 0) != 0 and "null batch" in hip.last_error()
    L.ba_select_destroy(None)
    one = np.ones(4, np.uint32)
    P = hip.SelectParamsC(*GOOD)
    assert not L.ba_select_create(None, *([one.ctypes.data] * 5), None, None, None, 1, 2) and "null argument" in hip.last_error()
    for k in range(5):   # (strand, support and exclude may be null)
        args = [one.ctypes.data] * 5
        args[k] = None
        assert not L.ba_select_create(ctypes.byref(P), *args, None, None, None, 1, 2) and "null argument" in hip.last_error(), k


def test_create_chained_refuses_a_null_batch_and_null_arguments(hip):
    L = hip.lib()
    one = np.zeros(4, np.uint32)
    P = hip.SelectParamsC(*GOOD)
    assert not L.ba_select_create_chained(ctypes.byref(P), None, one.ctypes.data, None, 1) and "null batch" in hip.last_error()
    assert not L.ba_select_create_chained(None, None, one.ctypes.data, None, 1) and "null argument" in hip.last_error()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_select_kernels_build_for_gfx950_without_scratch(tmp_path):
    csrc = os.path.join(ROOT, "block_aligner_amd", "csrc")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Rpass-analysis=kernel-resource-usage",
                        "-c", os.path.join(csrc, "ba_select.hip"), "-o", str(tmp_path / "ba_select.o")], capture_output=True, text=True)
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
    for k in ("k_select_group", "k_select_mark", "k_select_emit"):
        hits = [v for f, v in scratch.items() if k in f]
        assert hits == [0], (k, scratch)


def test_kernel_hash_and_makefile_list_the_select_sources():
    from tools import kernel_hash
    assert "ba_select.hip" in kernel_hash.FILES and "ba_select.h" in kernel_hash.FILES
    mk = open(os.path.join(ROOT, "block_aligner_amd", "csrc", "Makefile")).read()
    assert re.search(r"^XOBJS := .*\$\(OBJ\)/ba_select\.o", mk, flags=re.M) and re.search(r"^HDRS := .*\bba_select\.h\b", mk, flags=re.M)
    assert re.search(r"^\$\(OBJ\)/ba_select\.o: ba_select\.hip \$\(HDRS\)", mk, flags=re.M)


# ------------------------------------------------------------------ records (host only)
def test_sam_flags_of_the_known_answer(hip):
    f = hip.sam_flags(R.KNOWN_OUT["cls"], R.KNOWN["strand"])
    #            dropped  primary  suppl. minus  dropped  secondary  sec. minus  excluded  primary minus  dropped  secondary
    assert f.tolist() == [0, 0, 2048 + 16, 0, 256, 256 + 16, 0, 16, 0, 256]
    assert hip.sam_flags(R.KNOWN_OUT["cls"]).tolist() == [0, 0, 2048, 0, 256, 256, 0, 0, 0, 256]
    with pytest.raises(ValueError):
        hip.sam_flags([0, 1], [0])


def test_paf_lines_of_the_known_answer(hip):
    """The known answer as alignments: results and statistics made up so that paf_columns mirrors the minus-strand coordinates."""
    K = R.KNOWN
    n = len(K["read"])
    qs, qe = np.array(K["q_start"]), np.array(K["q_end"])
    results = dict(score=np.array(K["score"], np.int32), q_end=qe.astype(np.uint32), r_end=(5000 + qe).astype(np.uint32), status=np.zeros(n, np.uint32))
    stats = {"q_start": qs.astype(np.uint32), "r_start": (5000 + qs).astype(np.uint32), "matches": (qe - qs - 3).astype(np.uint32),
             "columns": (qe - qs + 1).astype(np.uint32), "mismatches": np.full(n, 2, np.uint32), "ins": np.full(n, 1, np.uint32), "del": np.full(n, 1, np.uint32)}
    paf = hip.paf_columns(results, stats, K["q_len"], K["strand"])
    sel = {k: np.array(v) for k, v in R.KNOWN_OUT.items()}
    cigars = [f"{e - s}M" for s, e in zip(K["q_start"], K["q_end"])]
    lines = hip.paf_lines(["read_a", b"read_b"], [1000, 400], "chr", 90000, paf, sel, cigars)
    assert lines == [
        "read_a\t1000\t0\t500\t+\tchr\t90000\t5000\t5500\t497\t501\t10\ttp:A:P\tNM:i:4\tAS:i:500\ts2:i:410\tcg:Z:500M",
        "read_a\t1000\t480\t980\t-\tchr\t90000\t5020\t5520\t497\t501\t20\ttp:A:P\tNM:i:4\tAS:i:480\ts2:i:300\tcg:Z:500M",
        "read_a\t1000\t100\t450\t+\tchr\t90000\t5100\t5450\t347\t351\t0\ttp:A:S\tNM:i:4\tAS:i:410\tcg:Z:350M",
        "read_a\t1000\t20\t420\t-\tchr\t90000\t5580\t5980\t397\t401\t0\ttp:A:S\tNM:i:4\tAS:i:405\tcg:Z:400M",
        "read_b\t400\t0\t400\t-\tchr\t90000\t5000\t5400\t397\t401\t0\ttp:A:P\tNM:i:4\tAS:i:200\ts2:i:200\tcg:Z:400M",
        "read_b\t400\t10\t390\t+\tchr\t90000\t5010\t5390\t377\t381\t0\ttp:A:S\tNM:i:4\tAS:i:200\tcg:Z:380M",
    ]
    bare = hip.paf_lines(["a", "b"], [1000, 400], "chr", 90000, paf, sel)   # no cg without cigars, s2 on heads only
    assert [len(ln.split("\t")) for ln in bare] == [16, 16, 15, 15, 16, 15] and not any("cg:Z" in ln for ln in bare)
    with pytest.raises(ValueError, match="one entry per read"):
        hip.paf_lines(["a"], [1000], "chr", 90000, paf, sel)
