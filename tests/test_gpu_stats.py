"""Per-alignment statistics on the MI355X (ba_*_stats): every field of every pair against a NumPy reference built here from the oracle's runs
and the raw sequences (uppercased for NucMatrix / AAMatrix batches) -- through every fill path, with and without CIGAR_EQ, in the special
start modes, for re-run pairs, sized batches, multibatches and extension batches -- and the refusals on the device."""
import zlib

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth, verify
from tests.test_gpu_extend import DNA_GAPS, NUC as EXT_NUC, SeedSet, composite, dna_seeds
from tests.test_gpu_multi import _flanked_pairs

pytestmark = pytest.mark.gpu

NUC = S.NucMatrix.new_simple(2, -3)
GAPS = (-5, -1)
FIELDS = ("q_start", "r_start", "columns", "matches", "mismatches", "positives", "ins", "del", "gap_opens", "longest_ins", "longest_del", "path_score")
FAILED = 1 | 2 | 4 | 8 | 16 | 32 | 128   # overflow, lost and watchdog bits: no record


def ref_stats(runs, q: bytes, r: bytes, matrix, gaps, query_idx: int, reference_idx: int, status: int = 0):
    """The record of one alignment from its runs and raw sequences, in NumPy."""
    rec = dict.fromkeys(FIELDS, 0)
    if status & FAILED:
        return rec
    runs = np.asarray(runs, dtype=np.int64)
    ops, lens = runs & 15, runs >> 4
    is_m = (ops >= 1) & (ops <= 3)
    i0 = query_idx - int(lens[is_m | (ops == 4)].sum())
    j0 = reference_idx - int(lens[is_m | (ops == 5)].sum())
    rec["q_start"], rec["r_start"] = i0, j0
    if runs.size == 0:
        return rec
    rep = np.repeat(ops, lens)
    di, dj = (rep != 5).astype(np.int64), (rep != 4).astype(np.int64)
    ipos, jpos = i0 + np.cumsum(di) - di, j0 + np.cumsum(dj) - dj
    mm = rep <= 3
    qa = np.frombuffer(q, np.uint8)[ipos[mm]].astype(np.int64)
    ra = np.frombuffer(r, np.uint8)[jpos[mm]].astype(np.int64)
    if getattr(matrix, "KIND", 1) != 2:   # NucMatrix / AAMatrix: the images hold the uppercased bytes
        qa, ra = verify._upper(qa), verify._upper(ra)
    s = verify.score_table(matrix)[qa, ra]
    gi, gd = lens[ops == 4], lens[ops == 5]
    rec.update({"columns": int(lens.sum()), "matches": int((qa == ra).sum()), "mismatches": int((qa != ra).sum()), "positives": int((s > 0).sum()),
                "ins": int(gi.sum()), "del": int(gd.sum()), "gap_opens": int(gi.size + gd.size), "longest_ins": int(gi.max(initial=0)),
                "longest_del": int(gd.max(initial=0)), "path_score": int(s.sum()) + int((gaps[0] + gaps[1] * (np.concatenate([gi, gd]) - 1)).sum())})
    return rec


def check_stats(st, want, what=""):
    for p, w in enumerate(want):
        got = {k: int(st[k][p]) for k in FIELDS}
        assert got == w, (what, p, got, w)
    cols = st["columns"].astype(np.float64)
    assert np.array_equal(st["identity"], np.divide(st["matches"], cols, out=np.zeros_like(cols), where=cols > 0))
    assert np.array_equal(st["edit_distance"], st["mismatches"] + st["ins"] + st["del"])


def flags_of(hip, mode):
    return sum({"trace": hip.TRACE, "x_drop": hip.X_DROP, "local_start": hip.LOCAL_START, "free_query_start_gaps": hip.FREE_QUERY_START_GAPS}[m] for m in mode)


def oracle_want(oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq):
    ref = oracle.batch_align(matrix, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, gaps, size, x_drop, mode, cigar_eq=cigar_eq, threads=8)
    want = []
    for p in range(len(pairs)):
        o = int(ref["cig_off"][p])
        runs = ref["cig_ops"][o:o + int(ref["cig_len"][p])]
        want.append(ref_stats(runs, pairs.query(p), pairs.reference(p), matrix, gaps, int(ref["query_idx"][p]), int(ref["reference_idx"][p])))
    return ref, want


def run_and_check(hip, oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq=False, kernel=None, what=""):
    flags = flags_of(hip, mode) | (hip.CIGAR_EQ if cigar_eq else 0)
    b = hip.BatchAligner(matrix, gaps, size, x_drop, flags, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    if kernel is not None:
        assert b.info()["kernel"] == kernel
    b.run()
    res = b.results()
    st = b.stats()
    runs, off = b.cigars(res["cigar_len"])
    b.close()
    assert not res["status"].any()
    ref, want = oracle_want(oracle, pairs, matrix, gaps, size, x_drop, mode, cigar_eq)
    assert np.array_equal(res["score"], ref["scores"]) and np.array_equal(res["cigar_len"], ref["cig_len"])
    check_stats(st, want, what)
    assert np.array_equal(st["path_score"], res["score"]), what
    for p in range(len(pairs)):   # the start is the one verify.check_cigar's walk implies
        cq, cr = verify.check_cigar(runs[int(off[p]):int(off[p + 1])], pairs.query(p), pairs.reference(p), matrix, gaps, int(res["score"][p]),
                                    int(res["query_idx"][p]), int(res["reference_idx"][p]), mode=mode, what=f"{what} {p}")
        assert (int(st["q_start"][p]), int(st["r_start"][p])) == (int(res["query_idx"][p]) - cq, int(res["reference_idx"][p]) - cr)
    return st, runs, off


# (size, development switch, kernel, pairs)
PATHS = {
    "k_small": ((32, 256), "BA_FORCE_SMALL", "k_small", lambda: synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=301, indels=2, indel_len=(10, 80))),
    "k_quad": ((32, 256), "BA_FORCE_QUAD", "k_quad", lambda: synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=302, indels=2, indel_len=(10, 80))),
    "k_multi128": ((128, 1024), "BA_FORCE_MULTI", "k_multi", lambda: synth.make_pairs(150, (800, 3000), (50, 300), 100, synth.DNA, seed=303, indels=3, indel_len=(20, 200))),
    "k_multi256": ((256, 2048), "BA_FORCE_MULTI", "k_multi", lambda: synth.make_pairs(150, (1500, 6000), (100, 600), 200, synth.DNA, seed=304, indels=3, indel_len=(20, 400))),
    "k_align": ((32, 256), None, "k_align", lambda: synth.make_pairs(300, (0, 2500), (0, 150), 40, synth.DNA, seed=305, indels=2, indel_len=(10, 80))),
    "row_tiled": ((128, 4096), None, None, lambda: synth.make_pairs(120, (3000, 9000), (100, 600), 100, synth.DNA, seed=306, indels=2, indel_len=(300, 1500))),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_dna_fill_paths(devlib, oracle, monkeypatch, path):
    """Every fill path, with and without CIGAR_EQ; the plain batch's matches / mismatches are the EQ batch's = / X cells, pair by pair."""
    hip = devlib
    size, env, kernel, make = PATHS[path]
    if env:
        monkeypatch.setenv(env, "1")
    pairs = make()
    x_drop = 400 if path == "row_tiled" else 100
    plain, _, _ = run_and_check(hip, oracle, pairs, NUC, GAPS, size, x_drop, ("trace", "x_drop"), False, kernel, path)
    eq, runs, off = run_and_check(hip, oracle, pairs, NUC, GAPS, size, x_drop, ("trace", "x_drop"), True, kernel, path + " eq")
    for p in range(len(pairs)):
        x = runs[int(off[p]):int(off[p + 1])].astype(np.int64)
        assert int(plain["matches"][p]) == int((x >> 4)[(x & 15) == 2].sum()), (path, p)
        assert int(plain["mismatches"][p]) == int((x >> 4)[(x & 15) == 3].sum()), (path, p)
    for k in FIELDS:
        assert np.array_equal(plain[k], eq[k]), k
    assert plain["mismatches"].sum() > 0 and plain["gap_opens"].sum() > 0


def test_protein_positives(hip, oracle):
    pairs = synth.make_pairs(300, (50, 1500), (0, 200), 20, synth.AMINO, seed=311, indels=1, indel_len=(5, 40))
    st, _, _ = run_and_check(hip, oracle, pairs, S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, ("trace", "x_drop"))
    assert (st["positives"] != st["matches"]).any() and (st["positives"] >= st["matches"]).all()


def _lowered(pairs, rng):
    pool = pairs.pool.copy()
    low = (rng.random(pool.size) < 0.3) & (pool >= 65) & (pool <= 90)
    pool[low] += 32
    return synth.PairSet(pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)


def test_byte_matrix_compares_raw_bytes(hip, oracle):
    """ByteMatrix images are the raw bytes: 'a' and 'A' differ."""
    pairs = _lowered(synth.make_pairs(200, (100, 1500), (0, 100), 10, synth.DNA, seed=312), np.random.default_rng(3))
    for eq in (False, True):
        st, _, _ = run_and_check(hip, oracle, pairs, S.BYTES1, (-2, -1), (32, 128), 0, ("trace",), eq)
        assert st["mismatches"].sum() > 0


@pytest.mark.parametrize("matrix", ["nuc", "aa"])
def test_lowercase_input(hip, oracle, matrix):
    rng = np.random.default_rng(313)
    if matrix == "nuc":
        pairs, m, g = synth.make_pairs(200, (100, 1500), (0, 100), 10, synth.DNA, seed=313), NUC, GAPS
    else:
        pairs, m, g = synth.make_pairs(200, (100, 900), (0, 90), 10, synth.AMINO, seed=314), S.static_matrix("BLOSUM62"), (-11, -1)
    for eq in (False, True):
        st, _, _ = run_and_check(hip, oracle, _lowered(pairs, rng), m, g, (32, 256), 50, ("trace", "x_drop"), eq)
        assert st["matches"].sum() > 0


@pytest.mark.parametrize("mode", [("trace", "local_start"), ("trace", "x_drop", "local_start"), ("trace", "free_query_start_gaps"),
                                  ("trace", "x_drop", "free_query_start_gaps")])
def test_local_and_free_start(hip, oracle, mode):
    pairs = _flanked_pairs(120, 315)
    st, _, _ = run_and_check(hip, oracle, pairs, NUC, GAPS, (32, 256), 80, mode, True)
    assert (st["r_start"] > 0).any()   # (flanked pairs: alignments that do not start at the origin)


def test_empty_sequences_and_pairs_without_runs(hip, oracle):
    rng = np.random.default_rng(316)
    lists = [(b"", b""), (b"", b"ACGT"), (b"ACGT", b""), (b"A", b"A"), (b"A", b"C"), (b"AAAAAAAAAAAA", b"CCCCCCCCCCCC"), (b"ACGTACGT", b"acgtacgt")]
    for _ in range(60):
        n = int(rng.integers(0, 600))
        a = synth.rand_str(rng, n, synth.DNA)
        b = synth.mutate(rng, a, int(rng.integers(0, 1 + n // 8)), synth.DNA) if n and rng.random() < 0.7 else synth.rand_str(rng, int(rng.integers(0, 600)), synth.DNA)
        lists.append((a.tobytes(), b.tobytes()))
    pairs = synth.PairSet.from_lists(lists)
    for mode, x in ((("trace", "x_drop"), 3), (("trace",), 0)):
        st, runs, off = run_and_check(hip, oracle, pairs, NUC, GAPS, (32, 256), x, mode, True)
        assert (np.diff(off) == 0).any()


def test_statistics_describe_the_rerun_pairs(devlib, oracle, monkeypatch):
    """Pairs re-run after the first pass (adaptive trace slots): the records describe the final runs, the ones cigars() returns."""
    hip = devlib
    monkeypatch.setenv("BA_ADAPTIVE_TRACE", "1")
    monkeypatch.setenv("BA_TRACE_MARGIN_PCT", "3")
    monkeypatch.setenv("BA_FORCE_TB", "1")
    pairs = synth.make_pairs(400, (800, 2500), (50, 250), 60, synth.DNA, seed=34, indels=3, indel_len=(30, 300))
    b = hip.BatchAligner(NUC, GAPS, (32, 512), 80, hip.TRACE | hip.X_DROP, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    b.run()
    assert b.retried() > 0
    res = b.results()
    st = b.stats()
    runs, off = b.cigars(res["cigar_len"])
    b.close()
    mine = [ref_stats(runs[int(off[p]):int(off[p + 1])], pairs.query(p), pairs.reference(p), NUC, GAPS, int(res["query_idx"][p]),
                      int(res["reference_idx"][p]), int(res["status"][p])) for p in range(len(pairs))]
    check_stats(st, mine, "own runs")
    _, want = oracle_want(oracle, pairs, NUC, GAPS, (32, 512), 80, ("trace", "x_drop"), False)
    check_stats(st, want, "oracle")


def test_sized_batch_in_caller_order(hip, oracle):
    pairs = synth.make_pairs(300, (200, 3000), (0, 200), 40, synth.DNA, seed=317, indels=2, indel_len=(10, 120))
    ranges = [(32, 256), (128, 1024), (32, 512)]
    sizes = np.array([ranges[p % 3] for p in range(len(pairs))], np.uint64)
    sb = hip.SizedBatchAligner(NUC, GAPS, 100, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, sizes=sizes)
    sb.run()
    st = sb.stats()
    sb.close()
    want = [None] * len(pairs)
    for k, rg in enumerate(ranges):
        idx = np.arange(k, len(pairs), 3)
        _, w = oracle_want(oracle, pairs.subset(idx), NUC, GAPS, rg, 100, ("trace", "x_drop"), True)
        for i, p in enumerate(idx):
            want[p] = w[i]
    check_stats(st, want, "sized")


def test_multibatch_in_caller_order(hip, oracle):
    pairs = synth.make_pairs(500, (0, 2500), (0, 200), 30, synth.DNA, seed=318)
    m = hip.MultiBatchAligner(NUC, GAPS, (32, 256), 70, hip.TRACE | hip.X_DROP, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, [0, 0])
    m.run()
    st = m.stats()
    m.close()
    _, want = oracle_want(oracle, pairs, NUC, GAPS, (32, 256), 70, ("trace", "x_drop"), False)
    check_stats(st, want, "multibatch")


def _check_extend(hip, oracle, m, gaps, size, x_drop, mode, ss):
    eb = hip.ExtendBatchAligner(m, gaps, size, x_drop, mode, *ss.args(), strand=ss.strand)
    eb.run()
    res = eb.results()
    st = eb.stats()
    eb.close()
    want = []
    for p in range(len(ss)):
        exp = composite(oracle, m, gaps, size, x_drop, mode, ss, p)
        assert int(res["q_start"][p]) == exp["q_start"] and int(res["q_end"][p]) == exp["q_end"]
        q, r = ss.q(p), ss.r(p)
        qa, ra = q[exp["q_start"]:exp["q_end"]], r[exp["r_start"]:exp["r_end"]]
        w = ref_stats(exp["runs"], qa, ra, m, gaps, len(qa), len(ra))
        assert (w["q_start"], w["r_start"]) == (0, 0)
        w["q_start"], w["r_start"] = exp["q_start"], exp["r_start"]
        want.append(w)
    check_stats(st, want, "extend")
    assert np.array_equal(st["path_score"], res["score"])
    return st


@pytest.mark.parametrize("strand", ["plus", "minus"])
def test_extension_dna(hip, oracle, strand):
    ss = dna_seeds(np.random.default_rng(zlib.crc32(strand.encode())), 300, lo=200, hi=6000, minus=strand == "minus")
    for mode in (hip.TRACE | hip.X_DROP, hip.TRACE | hip.X_DROP | hip.CIGAR_EQ):
        st = _check_extend(hip, oracle, EXT_NUC, DNA_GAPS, (32, 256), 100, mode, ss)
        assert st["gap_opens"].sum() > 0


def test_extension_protein(hip, oracle):
    rng = np.random.default_rng(319)
    seqs, qs, rs, sl = [], [], [], []
    for p in range(150):
        core = synth.rand_str(rng, int(rng.integers(100, 600)), synth.AMINO)
        mq = synth.mutate(rng, core, len(core) // 10, synth.AMINO)
        L = int(rng.integers(4, 12))
        a = int(rng.integers(0, min(len(mq), len(core)) - L))
        seqs += [mq.tobytes(), core.tobytes()]
        qs.append(min(a, len(mq) - L)); rs.append(a); sl.append(L)
    ss = SeedSet(seqs, list(range(0, 300, 2)), list(range(1, 300, 2)), qs, rs, sl)
    st = _check_extend(hip, oracle, S.static_matrix("BLOSUM62"), (-11, -1), (32, 256), 50, hip.TRACE | hip.X_DROP, ss)
    assert (st["positives"] != st["matches"]).any()


def test_reload_then_stats(hip, oracle):
    a = synth.make_pairs(300, (200, 2500), (0, 150), 40, synth.DNA, seed=320)
    c = synth.make_pairs(200, (100, 2000), (0, 200), 40, synth.DNA, seed=321)
    mode = hip.TRACE | hip.X_DROP
    b = hip.BatchAligner(NUC, GAPS, (32, 256), 100, mode, a.pool, a.q_off, a.q_len, a.r_off, a.r_len)
    b.run()
    b.stats()
    b.reload(c.pool, c.q_off, c.q_len, c.r_off, c.r_len)
    with pytest.raises(RuntimeError, match="has not finished a run"):
        b.stats()
    b.run()
    st = b.stats()
    b.close()
    _, want = oracle_want(oracle, c, NUC, GAPS, (32, 256), 100, ("trace", "x_drop"), False)
    check_stats(st, want, "reload")


def test_refusals_on_the_device(hip):
    pairs = synth.make_pairs(64, 600, 60, 30, synth.DNA, seed=7)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    b = hip.BatchAligner(NUC, GAPS, (32, 128), 100, hip.X_DROP, *args)
    b.run()
    with pytest.raises(RuntimeError, match="without BA_TRACE"):
        b.stats()
    b.close()
    b = hip.BatchAligner(NUC, GAPS, (32, 128), 100, hip.TRACE | hip.X_DROP, *args)
    with pytest.raises(RuntimeError, match="has not finished a run"):
        b.stats()
    b.launch()
    with pytest.raises(RuntimeError, match="launch in flight"):
        b.stats()
    b.wait()
    assert b.stats()["columns"].min() > 0 and b.stats_ms() > 0
    b.close()
    prof = [S.AAProfile.from_bytes(b"ACDEFGHIKLMN", 128, 2, -1, -5, 0, -5, -1) for _ in range(3)]
    pool = np.frombuffer(b"ACDEFGHKLMNACDEFGHIKLMNPQ", np.uint8)
    pb = hip.ProfileBatchAligner(prof, (32, 128), 0, hip.TRACE, pool, [0, 5, 10], [10, 12, 8])
    pb.run()
    with pytest.raises(RuntimeError, match="profile batch"):
        pb.stats()
    pb.close()
    ss = dna_seeds(np.random.default_rng(5), 20, lo=200, hi=800)
    eb = hip.ExtendBatchAligner(EXT_NUC, DNA_GAPS, (32, 256), 100, hip.X_DROP | hip.TRACE, *ss.args())
    with pytest.raises(RuntimeError, match="has not finished a run"):
        eb.stats()
    eb.close()
    eb = hip.ExtendBatchAligner(EXT_NUC, DNA_GAPS, (32, 256), 100, hip.X_DROP, *ss.args())
    eb.run()
    with pytest.raises(RuntimeError, match="without BA_TRACE"):
        eb.stats()
    eb.close()
