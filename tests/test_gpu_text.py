"""Alignment strings on the MI355X (ba_*_text): every pair's CIGAR, soft-clipped CIGAR, MD and cs against tests/text_ref.py rendered from the
oracle's runs and the raw sequences -- through the DNA fill paths, with and without CIGAR_EQ, X-drop, the special start modes, protein,
lowercase and N input, re-run pairs, sized batches, multibatches and extension batches on both strands -- cross-checked against stats()
and against the sequences themselves, and the refusals on the device."""
import ctypes
import re
import zlib

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import text_ref as T
from tests.test_gpu_extend import DNA_GAPS, NUC as EXT_NUC, SeedSet, composite, dna_seeds
from tests.test_gpu_multi import _flanked_pairs
from tests.test_gpu_stats import GAPS, NUC, _lowered, flags_of

pytestmark = pytest.mark.gpu

# (name, what, soft_clip)
WHATS = (("cigar", T.CIGAR, False), ("clip", T.CIGAR, True), ("md", T.MD, False), ("cs", T.CS, False))


def device_texts(hip, call, h, n, letters=True):
    """Every format by the two-call pattern (sizes, then text): the offsets of both calls agree; -> {name: [str per pair]}."""
    out = {}
    for name, w, clip in WHATS:
        if not letters and w != T.CIGAR:
            continue
        w |= hip.TEXT_SOFT_CLIP if clip else 0
        f = getattr(hip.lib(), call)
        sizes = np.zeros(n + 1, np.uint64)
        assert f(h, w, sizes.ctypes.data, None, 0) == 0, hip.last_error()
        buf = np.zeros(max(1, int(sizes[-1])), np.uint8)
        off = np.full(n + 1, 7, np.uint64)
        assert f(h, w, off.ctypes.data, buf.ctypes.data, int(sizes[-1])) == 0, hip.last_error()
        assert np.array_equal(sizes, off) and off[0] == 0 and (np.diff(off.astype(np.int64)) >= 0).all(), name
        out[name] = hip._text_list(buf[:int(off[-1])], off)
    return out


def expected(runs_of, q_of, r_of, q0, r0, status, letters=True):
    out = {}
    for name, w, clip in WHATS:
        if letters or w == T.CIGAR:
            out[name] = [T.render(w, runs_of(p), q_of(p), r_of(p), int(q0[p]), int(r0[p]), clip, int(status[p])) for p in range(len(q0))]
    return out


def compare(got, want, what=""):
    for name in want:
        for p, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (what, name, p, g, w)


def cross_checks(got, st, q_of, r_of, q_end, r_end, what=""):
    """MD's edits + the CIGAR's I = stats' edit distance; MD's counts + letters = the reference consumed; replaying cs rebuilds both segments."""
    for p, m in enumerate(got["md"]):
        if not m:
            assert got["cs"][p] == "" and got["cigar"][p] == ""
            continue
        eq, mis, dels = T.md_parts(m)
        ins = sum(int(n) for n in re.findall(r"([0-9]+)I", got["cigar"][p]))
        assert mis + dels + ins == int(st["edit_distance"][p]), (what, p)
        q0, r0 = int(st["q_start"][p]), int(st["r_start"][p])
        assert eq + mis + dels == int(r_end[p]) - r0, (what, p)
        q, r = q_of(p), r_of(p)
        assert T.cs_replay(got["cs"][p], r[r0:]) == (q[q0:int(q_end[p])], r[r0:int(r_end[p])]), (what, p)


def oracle_runs(oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq):
    ref = oracle.batch_align(matrix, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, gaps, size, x_drop, mode, cigar_eq=cigar_eq, threads=8)
    return ref, lambda p: ref["cig_ops"][int(ref["cig_off"][p]):int(ref["cig_off"][p]) + int(ref["cig_len"][p])]


def starts(runs_of, q_end, r_end):
    c = [T.consumed(runs_of(p)) for p in range(len(q_end))]
    return np.array([int(q_end[p]) - c[p][0] for p in range(len(c))]), np.array([int(r_end[p]) - c[p][1] for p in range(len(c))])


def check_batch(hip, oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq=False, kernel=None, what="", letters=True):
    flags = flags_of(hip, mode) | (hip.CIGAR_EQ if cigar_eq else 0)
    b = hip.BatchAligner(matrix, gaps, size, x_drop, flags, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    if kernel is not None:
        assert b.info()["kernel"] == kernel
    b.run()
    res = b.results()
    st = b.stats()
    got = device_texts(hip, "ba_batch_text", b._h, len(pairs), letters)
    assert b.text_ms() > 0 or not any(got["cigar"])
    b.close()
    ref, runs_of = oracle_runs(oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq)
    assert np.array_equal(res["score"], ref["scores"]) and np.array_equal(res["cigar_len"], ref["cig_len"])
    kind = T.kind_of(matrix)
    q_of = lambda p: T.image_letters(pairs.query(p), kind)   # noqa: E731
    r_of = lambda p: T.image_letters(pairs.reference(p), kind)   # noqa: E731
    q0, r0 = starts(runs_of, ref["query_idx"], ref["reference_idx"])
    want = expected(runs_of, q_of, r_of, q0, r0, res["status"], letters)
    compare(got, want, what)
    assert got["cigar"] == [hip.runs_to_string(runs_of(p)) for p in range(len(pairs))]
    if letters:
        cross_checks(got, st, q_of, r_of, res["query_idx"], res["reference_idx"], what)
    return got, st


PATHS = {
    "k_small": ((32, 256), "BA_FORCE_SMALL", "k_small", lambda: synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=401, indels=2, indel_len=(10, 80))),
    "k_quad": ((32, 256), "BA_FORCE_QUAD", "k_quad", lambda: synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=402, indels=2, indel_len=(10, 80))),
    "k_multi": ((128, 1024), "BA_FORCE_MULTI", "k_multi", lambda: synth.make_pairs(150, (800, 3000), (50, 300), 100, synth.DNA, seed=403, indels=3, indel_len=(20, 200))),
    "k_align": ((32, 256), None, "k_align", lambda: synth.make_pairs(300, (0, 2500), (0, 150), 40, synth.DNA, seed=405, indels=2, indel_len=(10, 80))),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_dna_fill_paths(devlib, oracle, monkeypatch, path):
    """Every DNA fill path, with and without CIGAR_EQ: MD and cs do not depend on it; X-drop stops before the ends (trailing S)."""
    hip = devlib
    size, env, kernel, make = PATHS[path]
    if env:
        monkeypatch.setenv(env, "1")
    pairs = make()
    plain, _ = check_batch(hip, oracle, pairs, NUC, GAPS, size, 100, ("trace", "x_drop"), False, kernel, path)
    eq, _ = check_batch(hip, oracle, pairs, NUC, GAPS, size, 100, ("trace", "x_drop"), True, kernel, path + " eq")
    assert plain["md"] == eq["md"] and plain["cs"] == eq["cs"]
    assert any(s.endswith("S") for s in plain["clip"]) and any("^" in s for s in plain["md"]) and any("+" in s for s in plain["cs"])


@pytest.mark.parametrize("mode", [("trace", "local_start"), ("trace", "x_drop", "free_query_start_gaps")])
def test_local_and_free_start(hip, oracle, mode):
    got, st = check_batch(hip, oracle, _flanked_pairs(120, 415), NUC, GAPS, (32, 256), 80, mode, True, what=str(mode))
    if "local_start" in mode:   # (a leading S where the query's start is skipped)
        assert any(re.match(r"[0-9]+S", s) for s in got["clip"]) and (st["q_start"] > 0).any()
    else:   # (FREE_QUERY_START_GAPS skips the reference's start: no S, but MD and cs start past r = 0)
        assert (st["r_start"] > 0).any()


def test_protein(hip, oracle):
    pairs = synth.make_pairs(200, (50, 1500), (0, 200), 20, synth.AMINO, seed=411, indels=1, indel_len=(5, 40))
    got, _ = check_batch(hip, oracle, pairs, S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, ("trace", "x_drop"), what="protein")
    letters = set("".join(got["md"])) - set("0123456789^")
    assert len(letters) > 4   # (AA letters, not only ACGT)


@pytest.mark.parametrize("matrix", ["nuc", "aa"])
def test_lowercase_input(hip, oracle, matrix):
    rng = np.random.default_rng(413)
    if matrix == "nuc":
        pairs, m, g = synth.make_pairs(150, (100, 1500), (0, 100), 10, synth.DNA, seed=413), NUC, GAPS
    else:
        pairs, m, g = synth.make_pairs(150, (100, 900), (0, 90), 10, synth.AMINO, seed=414), S.static_matrix("BLOSUM62"), (-11, -1)
    got, _ = check_batch(hip, oracle, _lowered(pairs, rng), m, g, (32, 256), 50, ("trace", "x_drop"), True, what="lower " + matrix)
    assert all(s == s.upper() for s in got["md"]) and all(s == s.lower() for s in got["cs"])


def test_n_bases(hip, oracle):
    pairs = synth.make_pairs(150, (100, 1500), (0, 100), 10, synth.DNA, seed=416)
    pool = pairs.pool.copy()
    pool[np.random.default_rng(416).random(pool.size) < 0.02] = ord("N")
    pairs = synth.PairSet(pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    got, _ = check_batch(hip, oracle, pairs, NUC, GAPS, (32, 256), 50, ("trace", "x_drop"), what="N")
    assert any("N" in s for s in got["md"]) and any("n" in s for s in got["cs"])


def test_byte_matrix_cigar_only(hip, oracle):
    pairs = _lowered(synth.make_pairs(150, (100, 1500), (0, 100), 10, synth.DNA, seed=417), np.random.default_rng(4))
    check_batch(hip, oracle, pairs, S.BYTES1, (-2, -1), (32, 128), 0, ("trace",), True, what="bytes", letters=False)
    b = hip.BatchAligner(S.BYTES1, (-2, -1), (32, 128), 0, hip.TRACE, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    b.run()
    for w in (hip.TEXT_MD, hip.TEXT_CS):
        with pytest.raises(RuntimeError, match="ByteMatrix"):
            b.text(w)
    b.close()


def test_profile_batch_cigar_only(hip):
    prof = [S.AAProfile.from_bytes(b"ACDEFGHIKLMN", 128, 2, -1, -5, 0, -5, -1) for _ in range(3)]
    pool = np.frombuffer(b"ACDEFGHKLMNACDEFGHIKLMNPQ", np.uint8)
    q_off, q_len = [0, 5, 10], [10, 12, 8]
    pb = hip.ProfileBatchAligner(prof, (32, 128), 0, hip.TRACE, pool, q_off, q_len)
    pb.run()
    res = pb.results()
    runs, off = pb.cigars(res["cigar_len"])
    for clip in (False, True):
        got = pb.text_list(hip.TEXT_CIGAR, soft_clip=clip)
        for p in range(3):
            x = runs[int(off[p]):int(off[p + 1])]
            q0 = int(res["query_idx"][p]) - T.consumed(x)[0]
            assert got[p] == T.cigar(x, q0, q_len[p], clip), (p, clip)
    for w in (hip.TEXT_MD, hip.TEXT_CS):
        with pytest.raises(RuntimeError, match="profile batch"):
            pb.text(w)
    pb.close()


def test_empty_sequences_and_pairs_without_runs(hip, oracle):
    rng = np.random.default_rng(418)
    lists = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"AAAAAAAAAAAA", b"CCCCCCCCCCCC"), (b"ACGTACGT", b"acgtacgt")]
    for _ in range(60):
        n = int(rng.integers(0, 600))
        a = synth.rand_str(rng, n, synth.DNA)
        b = synth.mutate(rng, a, int(rng.integers(0, 1 + n // 8)), synth.DNA) if n and rng.random() < 0.7 else synth.rand_str(rng, int(rng.integers(0, 600)), synth.DNA)
        lists.append((a.tobytes(), b.tobytes()))
    pairs = synth.PairSet.from_lists(lists)
    for mode, x in ((("trace", "x_drop"), 3), (("trace",), 0)):
        got, _ = check_batch(hip, oracle, pairs, NUC, GAPS, (32, 256), x, mode, True, what=str(mode))
        assert "" in got["md"] and "" in got["cigar"]


def test_rerun_pairs(devlib, oracle, monkeypatch):
    """Pairs re-run after the first pass (adaptive trace slots): the strings are those of the final runs."""
    hip = devlib
    monkeypatch.setenv("BA_ADAPTIVE_TRACE", "1")
    monkeypatch.setenv("BA_TRACE_MARGIN_PCT", "3")
    monkeypatch.setenv("BA_FORCE_TB", "1")
    pairs = synth.make_pairs(400, (800, 2500), (50, 250), 60, synth.DNA, seed=34, indels=3, indel_len=(30, 300))
    b = hip.BatchAligner(NUC, GAPS, (32, 512), 80, hip.TRACE | hip.X_DROP, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    b.run()
    assert b.retried() > 0
    res = b.results()
    runs, off = b.cigars(res["cigar_len"])
    got = device_texts(hip, "ba_batch_text", b._h, len(pairs))
    b.close()
    own = lambda p: runs[int(off[p]):int(off[p + 1])]   # noqa: E731
    q_of = lambda p: T.image_letters(pairs.query(p))   # noqa: E731
    r_of = lambda p: T.image_letters(pairs.reference(p))   # noqa: E731
    q0, r0 = starts(own, res["query_idx"], res["reference_idx"])
    compare(got, expected(own, q_of, r_of, q0, r0, res["status"]), "own runs")
    _, runs_of = oracle_runs(oracle, pairs, NUC, GAPS, (32, 512), 80, ("trace", "x_drop"), False)
    q0, r0 = starts(runs_of, res["query_idx"], res["reference_idx"])
    compare(got, expected(runs_of, q_of, r_of, q0, r0, res["status"]), "oracle")


def _caller_order_want(oracle, pairs, groups):
    """{name: [str]} in the caller's order; groups: [(caller indices, size range)] each aligned by the oracle on its own."""
    want = {name: [None] * len(pairs) for name, _, _ in WHATS}
    for idx, rg, mode, eq in groups:
        sub = pairs.subset(idx)
        ref, runs_of = oracle_runs(oracle, sub, NUC, GAPS, rg, mode[1], mode[0], eq)
        q0, r0 = starts(runs_of, ref["query_idx"], ref["reference_idx"])
        w = expected(runs_of, lambda p: T.image_letters(sub.query(p)), lambda p: T.image_letters(sub.reference(p)), q0, r0, np.zeros(len(sub), np.uint32))
        for name in w:
            for i, p in enumerate(idx):
                want[name][p] = w[name][i]
    return want


def test_sized_batch_in_caller_order(hip, oracle):
    pairs = synth.make_pairs(300, (200, 3000), (0, 200), 40, synth.DNA, seed=419, indels=2, indel_len=(10, 120))
    ranges = [(32, 256), (128, 1024), (32, 512)]
    sizes = np.array([ranges[p % 3] for p in range(len(pairs))], np.uint64)
    sb = hip.SizedBatchAligner(NUC, GAPS, 100, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, sizes=sizes)
    sb.run()
    got = device_texts(hip, "ba_sized_batch_text", sb._h, len(pairs))
    assert sb.text_list(hip.TEXT_MD) == got["md"]
    sb.close()
    want = _caller_order_want(oracle, pairs, [(np.arange(k, len(pairs), 3), rg, (("trace", "x_drop"), 100), True) for k, rg in enumerate(ranges)])
    compare(got, want, "sized")


def test_multibatch_in_caller_order(hip, oracle):
    pairs = synth.make_pairs(500, (0, 2500), (0, 200), 30, synth.DNA, seed=420)
    m = hip.MultiBatchAligner(NUC, GAPS, (32, 256), 70, hip.TRACE | hip.X_DROP, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, [0, 0])
    m.run()
    got = device_texts(hip, "ba_multibatch_text", m._h, len(pairs))
    st = m.stats()
    res = m.results()
    m.close()
    compare(got, _caller_order_want(oracle, pairs, [(np.arange(len(pairs)), (32, 256), (("trace", "x_drop"), 70), False)]), "multibatch")
    cross_checks(got, st, lambda p: T.image_letters(pairs.query(p)), lambda p: T.image_letters(pairs.reference(p)), res["query_idx"], res["reference_idx"])


def _check_extend(hip, oracle, m, gaps, size, x_drop, mode, ss, what):
    eb = hip.ExtendBatchAligner(m, gaps, size, x_drop, mode, *ss.args(), strand=ss.strand)
    eb.run()
    res = eb.results()
    st = eb.stats()
    got = device_texts(hip, "ba_extend_batch_text", eb._h, len(ss))
    eb.close()
    kind = T.kind_of(m)
    q_of = lambda p: T.image_letters(ss.seqs[ss.q_idx[p]], kind, ss.strand is not None and bool(ss.strand[p]))   # noqa: E731
    r_of = lambda p: T.image_letters(ss.seqs[ss.r_idx[p]], kind)   # noqa: E731
    exps = [composite(oracle, m, gaps, size, x_drop, mode, ss, p) for p in range(len(ss))]
    assert [e["q_start"] for e in exps] == res["q_start"].tolist()
    want = expected(lambda p: exps[p]["runs"], q_of, r_of, [e["q_start"] for e in exps], [e["r_start"] for e in exps], res["status"])
    compare(got, want, what)
    cross_checks(got, st, q_of, r_of, res["q_end"], res["r_end"], what)
    return got


@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_extension_dna(hip, oracle, strand):
    ss = dna_seeds(np.random.default_rng(zlib.crc32(b"text" + strand.encode())), 200, lo=200, hi=5000, minus=strand == "minus")
    for mode in (hip.TRACE | hip.X_DROP, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ):
        got = _check_extend(hip, oracle, EXT_NUC, DNA_GAPS, (32, 256), 100, mode, ss, strand)
        assert any(s.endswith("S") for s in got["clip"]) and any(re.match(r"[0-9]+S", s) for s in got["clip"])
    if strand == "minus":
        assert ss.strand.any()


def test_extension_protein(hip, oracle):
    rng = np.random.default_rng(421)
    seqs, qs, rs, sl = [], [], [], []
    for p in range(120):
        core = synth.rand_str(rng, int(rng.integers(100, 600)), synth.AMINO)
        mq = synth.mutate(rng, core, len(core) // 10, synth.AMINO)
        L = int(rng.integers(4, 12))
        a = int(rng.integers(0, min(len(mq), len(core)) - L))
        seqs += [mq.tobytes(), core.tobytes()]
        qs.append(min(a, len(mq) - L)); rs.append(a); sl.append(L)
    ss = SeedSet(seqs, list(range(0, 240, 2)), list(range(1, 240, 2)), qs, rs, sl)
    _check_extend(hip, oracle, S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, hip.TRACE | hip.X_DROP, ss, "protein")


def test_reload_then_text(hip, oracle):
    a = synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=422)
    c = synth.make_pairs(200, (100, 2000), (0, 200), 40, synth.DNA, seed=423)
    mode = hip.TRACE | hip.X_DROP
    b = hip.BatchAligner(NUC, GAPS, (32, 256), 100, mode, a.pool, a.q_off, a.q_len, a.r_off, a.r_len)
    b.run()
    before = b.text_list(hip.TEXT_MD)
    b.reload(c.pool, c.q_off, c.q_len, c.r_off, c.r_len)
    with pytest.raises(RuntimeError, match="has not finished a run"):
        b.text(hip.TEXT_MD)
    b.run()
    got = b.text_list(hip.TEXT_MD)   # (the sizes kept for the first set's run are not reused)
    b.close()
    ref, runs_of = oracle_runs(oracle, c, NUC, GAPS, (32, 256), 100, ("trace", "x_drop"), False)
    q0, r0 = starts(runs_of, ref["query_idx"], ref["reference_idx"])
    want = [T.md(runs_of(p), T.image_letters(c.query(p)), T.image_letters(c.reference(p)), int(q0[p]), int(r0[p])) for p in range(len(c))]
    assert got == want and len(before) == 300


def test_refusals_on_the_device(hip):
    pairs = synth.make_pairs(64, 600, 60, 30, synth.DNA, seed=7)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    f = hip.lib().ba_batch_text
    b = hip.BatchAligner(NUC, GAPS, (32, 128), 100, hip.X_DROP, *args)
    b.run()
    with pytest.raises(RuntimeError, match="without BA_TRACE"):
        b.text(hip.TEXT_CIGAR)
    b.close()
    b = hip.BatchAligner(NUC, GAPS, (32, 128), 100, hip.TRACE | hip.X_DROP, *args)
    with pytest.raises(RuntimeError, match="has not finished a run"):
        b.text(hip.TEXT_CIGAR)
    b.launch()
    with pytest.raises(RuntimeError, match="launch in flight"):
        b.text(hip.TEXT_CIGAR)
    b.wait()
    off = np.zeros(65, np.uint64)
    assert f(b._h, hip.TEXT_MD, None, None, 0) != 0 and "null argument" in hip.last_error()
    for bad in (3, 0x80, hip.TEXT_MD | 0x10000):
        assert f(b._h, bad, off.ctypes.data, None, 0) != 0 and "unknown what" in hip.last_error()
    for w in (hip.TEXT_MD, hip.TEXT_CS):
        assert f(b._h, w | hip.TEXT_SOFT_CLIP, off.ctypes.data, None, 0) != 0 and "SOFT_CLIP" in hip.last_error()
    buf, want_off = b.text(hip.TEXT_CS)
    assert buf.size > 10 and b.text_ms() > 0
    small = np.zeros(buf.size - 1, np.uint8)
    off[:] = 0
    assert f(b._h, hip.TEXT_CS, off.ctypes.data, small.ctypes.data, small.size) != 0
    assert "too small" in hip.last_error() and str(buf.size) in hip.last_error()
    assert np.array_equal(off, want_off)   # (the offsets are filled)
    assert f(b._h, hip.TEXT_CS, off.ctypes.data, small.ctypes.data, ctypes.c_uint64(small.size)) != 0
    b.close()
    ss = dna_seeds(np.random.default_rng(5), 20, lo=200, hi=800)
    eb = hip.ExtendBatchAligner(EXT_NUC, DNA_GAPS, (32, 256), 100, hip.X_DROP | hip.TRACE, *ss.args())
    with pytest.raises(RuntimeError, match="has not finished a run"):
        eb.text(hip.TEXT_CIGAR)
    eb.close()
    eb = hip.ExtendBatchAligner(EXT_NUC, DNA_GAPS, (32, 256), 100, hip.X_DROP, *ss.args())
    eb.run()
    with pytest.raises(RuntimeError, match="without BA_TRACE"):
        eb.text(hip.TEXT_CIGAR)
    eb.close()
