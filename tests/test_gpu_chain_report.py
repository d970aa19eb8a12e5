"""Statistics and strings of chain batches on the MI355X (ChainBatchAligner.report()): every field and every string of every chain against
tests/test_gpu_stats.py::ref_stats and tests/text_ref.py::render over the model's expected runs (tests/chain_ref.py over the oracle), none
left out; K = 1 against the extension batch bit for bit; the element counts around the wave's chunks; missing inner batches, reloads,
re-runs and the refusals. (tests/test_gpu_stats.py has no way to make a pair fail at these sizes -- its development switches force fill
paths and re-runs, which end with status 0 --, so the zero record of a failed chain is the CPU model's: tests/test_chain_report_ref.py.)"""
import ctypes

import numpy as np
import pytest

from tests import chain_ref as R, chain_report_ref as M, text_ref as T
from tests.test_gpu_chain import expected
from tests.test_gpu_stats import check_stats

pytestmark = pytest.mark.gpu

FORMATS = (("cigar", T.CIGAR, False), ("clip", T.CIGAR, True), ("md", T.MD, False), ("cs", T.CS, False))


@pytest.fixture(scope="module")
def sets():
    return R.dna_sets()


def want_of(cs, cfg, exps):
    """-> (records, {format: [str]}) the report must give for the model's expected results."""
    m, gaps = cfg["m"], cfg["gaps"]
    kind = T.kind_of(m)
    recs = [M.whole_record(exp, m, gaps, cs.q(c), cs.r(c)) for c, exp in enumerate(exps)]
    texts = {}
    for name, what, clip in FORMATS:
        if kind == "bytes" and what != T.CIGAR:
            continue
        texts[name] = [T.render(what, exp["runs"], T.image_letters(cs.q(c), kind), T.image_letters(cs.r(c), kind), exp["q_start"], exp["r_start"], clip)
                       for c, exp in enumerate(exps)]
    return recs, texts


def check_report(hip, cb, cs, cfg, exps, what=""):
    """After cb.run(): every chain of the set."""
    res = cb.results()
    assert not res["status"].any(), what
    rep = cb.report()
    st = rep.stats()
    recs, texts = want_of(cs, cfg, exps)
    check_stats(st, recs, what)
    assert np.array_equal(st["path_score"], res["score"]), what
    assert np.array_equal(st["q_start"], res["q_start"]) and np.array_equal(st["r_start"], res["r_start"]), what
    assert np.array_equal(st["matches"] + st["mismatches"] + st["ins"] + st["del"], st["columns"]), what
    for name, fmt, clip in FORMATS:
        if name in texts:
            got = rep.text_list(fmt, clip)
            assert len(got) == len(cs)
            for c, (g, w) in enumerate(zip(got, texts[name])):
                assert g == w, (what, name, c, g[:200], w[:200])
    runs, off = cb.cigars(res["cigar_len"])
    assert texts["cigar"] == [hip.runs_to_string(runs[int(off[c]):int(off[c + 1])]) for c in range(len(cs))]
    return st, texts


def run_and_check(hip, oracle, cs, cfg, mode, key=None, what=""):
    cb = hip.ChainBatchAligner(cfg["m"], cfg["gaps"], cfg["size"], cfg["x_drop"], mode, *cs.args(), strand=cs.strand)
    cb.run()
    exps = expected(oracle, cfg["m"], cfg["gaps"], cfg["size"], cfg["x_drop"], mode, cs, key)
    out = check_report(hip, cb, cs, cfg, exps, what)
    s_ms, t_ms = cb.report().ms()
    assert s_ms > 0 and t_ms > 0
    times = cb.times()
    cb.close()
    return out + (times,)


@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("name", ["mixed", "dense", "minus"])
def test_dna_sets(hip, oracle, sets, name, eq):
    mode = hip.TRACE | hip.X_DROP | (hip.CIGAR_EQ if eq else 0)
    st, texts, _ = run_and_check(hip, oracle, sets[name], M.DNA, mode, key=name, what=name)
    assert st["mismatches"].sum() and st["ins"].sum() and st["del"].sum() and st["gap_opens"].sum()
    assert any(s.endswith("S") for s in texts["clip"]) and any(s.split("S")[0].isdigit() for s in texts["clip"])
    if name == "minus":
        assert sets[name].strand.sum() > 20


def test_protein(hip, oracle):
    st, texts, _ = run_and_check(hip, oracle, M.protein_set(), M.PROTEIN, hip.TRACE | hip.X_DROP, what="protein")
    assert (st["positives"] != st["matches"]).any() and set(texts) == {"cigar", "clip", "md", "cs"}


def test_bytes(hip, oracle):
    cs = M.bytes_set()
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    st, texts, _ = run_and_check(hip, oracle, cs, M.BYTES, mode, what="bytes")
    assert set(texts) == {"cigar", "clip"} and st["mismatches"].sum()
    cb = hip.ChainBatchAligner(M.BYTES["m"], M.BYTES["gaps"], M.BYTES["size"], M.BYTES["x_drop"], mode, *cs.args())
    cb.run()
    for fmt in (hip.TEXT_MD, hip.TEXT_CS):
        with pytest.raises(RuntimeError, match="MD and cs are letter formats, and a ByteMatrix batch compares raw bytes"):
            cb.report().text(fmt)
    cb.close()


@pytest.mark.parametrize("eq", [False, True])
def test_one_anchor_equals_the_extension_batch(hip, sets, eq):
    """K = 1 is a seed: ExtendBatchAligner's records and texts on the same seeds, bit for bit."""
    mode = hip.TRACE | hip.X_DROP | (hip.CIGAR_EQ if eq else 0)
    cs = sets["mixed"].first_anchor_seeds()
    cb = hip.ChainBatchAligner(M.NUC, M.DNA["gaps"], (32, 256), 100, mode, *cs.args(), strand=cs.strand)
    eb = hip.ExtendBatchAligner(M.NUC, M.DNA["gaps"], (32, 256), 100, mode, cs.pool, cs.q_off, cs.q_len, cs.r_off, cs.r_len, cs.q_anchor, cs.r_anchor,
                                cs.anchor_len, strand=cs.strand)
    cb.run(); eb.run()
    assert not eb.results()["status"].any() and not cb.results()["status"].any()
    got, want = cb.report().stats(), eb.stats()
    assert list(got) == list(want) and want["columns"].sum() > 0
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    for _, fmt, clip in FORMATS:
        (b1, o1), (b2, o2) = cb.report().text(fmt, clip), eb.text(fmt, clip)
        assert np.array_equal(o1, o2) and np.array_equal(b1, b2) and len(b2)
    cb.close(); eb.close()


@pytest.mark.parametrize("eq", [False, True])
def test_element_counts_around_the_chunks(hip, oracle, eq):
    """K in {1, 2, 31, 32, 33, 63, 64, 65, 130}, one anchor of 300 columns, 130 adjacent exact anchors."""
    cs = M.boundary_set()
    mode = hip.TRACE | hip.X_DROP | (hip.CIGAR_EQ if eq else 0)
    st, _, _ = run_and_check(hip, oracle, cs, M.DNA, mode, what="boundary")
    long_anchor = len(M.BOUNDARY_K)
    assert int(st["mismatches"][long_anchor]) >= 3 and int(st["columns"][long_anchor]) >= 300
    assert int(st["matches"][-1]) >= 650


@pytest.mark.parametrize("eq", [False, True])
def test_gap_pieces_of_more_than_64_runs(hip, oracle, eq):
    cs = M.wide_gap_chain(eq)
    mode = hip.TRACE | hip.X_DROP | (hip.CIGAR_EQ if eq else 0)
    cfg = dict(M.DNA, size=(32, 128))
    st, _, _ = run_and_check(hip, oracle, cs, cfg, mode, what="wide gaps")
    assert int(st["gap_opens"][0]) > 64 or int(st["mismatches"][0]) > 64


def test_without_ends_the_ends_batch_is_null(hip, oracle, sets):
    cs = R.without_ends(sets["mixed"], 60)
    st, _, times = run_and_check(hip, oracle, cs, M.DNA, hip.TRACE | hip.X_DROP, what="no ends")
    assert times["ends_ms"] == 0 and times["gaps_ms"] > 0 and not st["q_start"].any()


def test_without_aligned_gaps_the_gaps_batch_is_null(hip, oracle):
    cs = M.no_aligned_gap_set()
    st, _, times = run_and_check(hip, oracle, cs, M.DNA, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ, what="no aligned gaps")
    assert times["gaps_ms"] == 0 and times["ends_ms"] > 0 and st["gap_opens"].sum() > 0


def test_reload_and_rerun(hip, oracle, sets):
    """The statistics and all three strings follow the loaded set; a second run() gives the same text."""
    mode = hip.TRACE | hip.X_DROP | hip.CIGAR_EQ
    big = sets["mixed"]
    idx = range(10, 50)
    small = big.subset(idx)
    cfg = M.DNA
    exps = expected(oracle, cfg["m"], cfg["gaps"], cfg["size"], cfg["x_drop"], mode, big, "mixed")
    cb = hip.ChainBatchAligner(cfg["m"], cfg["gaps"], cfg["size"], cfg["x_drop"], mode, *big.args(), strand=big.strand)
    rep = cb.report()
    cb.run()
    check_report(hip, cb, big, cfg, exps, "first load")
    cb.reload(*small.args(), strand=small.strand)
    with pytest.raises(RuntimeError, match=r"has not finished a run \(ba_chain_batch_run\)"):
        rep.stats()
    with pytest.raises(RuntimeError, match=r"has not finished a run \(ba_chain_batch_run\)"):
        rep.text()
    cb.run()
    check_report(hip, cb, small, cfg, [exps[c] for c in idx], "smaller set")
    cb.reload(*big.args(), strand=big.strand)
    cb.run()
    _, texts = check_report(hip, cb, big, cfg, exps, "back")
    cb.run()
    for name, fmt, clip in FORMATS:
        assert rep.text_list(fmt, clip) == texts[name], name
    cb.close()


def test_refusals_on_the_device(hip, sets):
    cs = sets["mixed"].subset(range(20))
    args = (M.NUC, M.DNA["gaps"], (32, 256), 100)
    cb = hip.ChainBatchAligner(*args, hip.X_DROP, *cs.args())
    cb.run()
    with pytest.raises(RuntimeError, match="created without BA_TRACE"):
        cb.report().stats()
    with pytest.raises(RuntimeError, match="created without BA_TRACE"):
        cb.report().text()
    cb.close()
    cb = hip.ChainBatchAligner(*args, hip.X_DROP | hip.TRACE, *cs.args())
    rep = cb.report()
    with pytest.raises(RuntimeError, match=r"stats: the batch has not finished a run \(ba_chain_batch_run\)"):
        rep.stats()
    with pytest.raises(RuntimeError, match=r"text: the batch has not finished a run \(ba_chain_batch_run\)"):
        rep.text()
    assert rep.ms() == (0.0, 0.0)
    cb.run()
    L = hip.lib()
    assert L.ba_chain_batch_stats(cb._h, None) != 0 and "null argument" in hip.last_error()
    assert L.ba_chain_batch_text(cb._h, hip.TEXT_CIGAR, None, None, 0) != 0 and "null argument" in hip.last_error()
    with pytest.raises(RuntimeError, match="BA_TEXT_SOFT_CLIP goes with BA_TEXT_CIGAR only"):
        rep.text(hip.TEXT_MD, True)
    with pytest.raises(RuntimeError, match="unknown what"):
        rep.text(7)
    buf, off = rep.text(hip.TEXT_CS)
    total = int(off[-1])
    assert total == buf.size and total > 0
    short = np.zeros(total - 1, np.uint8)
    off2 = np.zeros(len(cs) + 1, np.uint64)
    assert L.ba_chain_batch_text(cb._h, hip.TEXT_CS, off2.ctypes.data, short.ctypes.data, short.size) != 0
    assert f"text buffer too small: the text needs {total} bytes, the buffer holds {total - 1}" in hip.last_error()
    assert np.array_equal(off2, off)   # (the offsets are filled)
    s_ms, t_ms = ctypes.c_float(), ctypes.c_float()
    assert L.ba_chain_batch_report_ms(cb._h, None, ctypes.byref(t_ms)) == 0 and L.ba_chain_batch_report_ms(cb._h, ctypes.byref(s_ms), None) == 0
    cb.close()
