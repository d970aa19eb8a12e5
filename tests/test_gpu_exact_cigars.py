"""Optimal alignment paths of the exact full-matrix DP on the MI355X (ba_*_exact_cigars): the runs of every pair byte for byte against the
numpy / Python walk of tests/exact_path.py, tie-heavy inputs, one larger case through verify.check_cigar, pair selection and batch types,
the two-call pattern, BA_CIGAR_EQ, the refusals, and the use case: the exact path of pairs the block heuristic got wrong."""
import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from block_aligner_amd.verify import check_cigar
from tests import exact_dp, exact_path, gotoh
from tests.test_gpu_exact import BYTES, FIELDS, GAPS, NUC, batch, kinds, records, related, seed_set

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 7, 8, 9, 63, 64, 65, 127, 128, 129, 191)
REQUESTS = {"global": ("global", -1), "extend": ("extend", -1), "extend_x0": ("extend", 0), "extend_x30": ("extend", 30)}
_sets = {}


def what_of(hip, name):
    return hip.EXACT_GLOBAL if name == "global" else hip.EXACT_EXTEND


def length_pairs(kind):
    """nuc: every ordered pair of LENGTHS, one in four with a lowercase query; aa and bytes: 40 of them in a seeded order. Built once."""
    if kind not in _sets:
        rng = np.random.default_rng({"nuc": 300, "aa": 301, "bytes": 302}[kind])
        combos = [(a, b) for a in LENGTHS for b in LENGTHS]
        if kind != "nuc":
            combos = [combos[k] for k in rng.permutation(len(combos))[:40]]
        alphabet = kinds()[kind][2]
        _sets[kind] = synth.PairSet.from_lists([related(rng, a, b, alphabet, lower=(kind != "bytes" and n % 4 == 0)) for n, (a, b) in enumerate(combos)])
    return _sets[kind]


def split(runs, off):
    return [[int(x) for x in runs[int(off[k]):int(off[k + 1])]] for k in range(len(off) - 1)]


def helper(pairs, m, gaps, what, x_drop, eq=False, which=None):
    out = [exact_path.exact_runs(pairs.query(int(p)), pairs.reference(int(p)), m, gaps, what, x_drop, eq) for p in (range(len(pairs)) if which is None else which)]
    return [r for r, _ in out], [c for _, c in out]


# ---------------------------------------------------------------- 1. byte-identical to the helper
@pytest.mark.parametrize("request_name", sorted(REQUESTS))
@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_runs_equal_helper(hip, kind, request_name):
    m, gaps, _a = kinds()[kind]
    pairs = length_pairs(kind)
    what, x_drop = REQUESTS[request_name]
    b = batch(hip, m, gaps, pairs)
    rec, runs, off = b.exact_cigars(what_of(hip, what), x_drop)
    ex = b.exact(what_of(hip, what), x_drop)
    b.close()
    want_rec, want_runs = helper(pairs, m, gaps, what, x_drop)
    assert records(rec) == records(ex) == want_rec
    got = split(runs, off)
    bad = [p for p in range(len(pairs)) if got[p] != want_runs[p]]
    assert not bad, (bad[:5], got[bad[0]], want_runs[bad[0]])
    assert int(off[-1]) == len(runs) == sum(len(c) for c in want_runs)
    if kind == "nuc":
        assert len(pairs) == len(LENGTHS) ** 2
    if request_name == "global":                      # (a path to the corner has gaps of both kinds among these lengths)
        assert any(4 in {x & 15 for x in c} for c in got) and any(5 in {x & 15 for x in c} for c in got)


# ---------------------------------------------------------------- 2. tie-heavy inputs
@pytest.mark.parametrize("gaps", [(-2, -1), (-1, -1)])
def test_tie_heavy_inputs(hip, gaps):
    """(-1, -1) is a linear gap cost: such a batch is built for the exact calls, and a launch of the block kernels is refused with the
    reference's message (they need open < extend)."""
    rng = np.random.default_rng(310)
    lists = []
    for n in (64, 65, 130):
        for d in (0, 1, 3, 17):
            lists += [(b"A" * n, b"A" * (n - d)), (b"A" * (n - d), b"A" * n)]
            two = synth.rand_str(rng, n, np.frombuffer(b"AC", np.uint8))
            lists += [(two.tobytes(), synth.rand_str(rng, n - d, np.frombuffer(b"AC", np.uint8)).tobytes()), (two[d:].tobytes(), two[:n - d].tobytes())]
    pairs = synth.PairSet.from_lists(lists)
    m = S.NucMatrix.new_simple(1, -1)
    b = batch(hip, m, gaps, pairs)
    for what, x_drop in (("global", -1), ("extend", -1), ("extend", 3)):
        rec, runs, off = b.exact_cigars(what_of(hip, what), x_drop)
        want_rec, want_runs = helper(pairs, m, gaps, what, x_drop)
        assert records(rec) == want_rec
        assert split(runs, off) == want_runs, (what, x_drop)
    if gaps[0] == gaps[1]:
        with pytest.raises(RuntimeError, match="Gap open must cost more than gap extend"):
            b.run()
        with pytest.raises(RuntimeError, match="Gap open must cost more than gap extend"):      # extension batches stay strict
            ss = seed_set()
            hip.ExtendBatchAligner(m, gaps, (32, 256), 60, hip.X_DROP, *ss.args(), strand=ss.strand)
    b.close()


# ---------------------------------------------------------------- 3. one larger case
@pytest.mark.parametrize("what", ["global", "extend"])
def test_larger_pairs(hip, what):
    rng = np.random.default_rng(320)
    lens = [(2000, 1500), (1500, 2000), (2000, 2000), (1999, 1473)] + [tuple(int(x) for x in rng.integers(600, 2000, 2)) for _ in range(20)]
    pairs = synth.PairSet.from_lists([related(rng, a, b, synth.DNA) for a, b in lens])
    assert len(pairs) == 24
    b = batch(hip, NUC, GAPS, pairs, mode=hip.CIGAR_EQ)
    rec, runs, off = b.exact_cigars(what_of(hip, what), -1)
    b.close()
    got = split(runs, off)
    for p in range(len(pairs)):
        q, r = pairs.query(p), pairs.reference(p)
        want = gotoh.global_score(q, r, NUC, GAPS) if what == "global" else exact_dp.exact_extend(q, r, NUC, GAPS)[0]
        assert int(rec["score"][p]) == want, p
        check_cigar(got[p], q, r, NUC, GAPS, int(rec["score"][p]), int(rec["query_idx"][p]), int(rec["reference_idx"][p]), what=p)
        assert {x & 15 for x in got[p]} <= {2, 3, 4, 5}


# ---------------------------------------------------------------- 4. pair selection, batch types, the two-call pattern
def test_selection_and_batch_types(hip):
    pairs = synth.make_pairs(60, (0, 500), (0, 40), 20, synth.DNA, seed=330, indels=1, indel_len=(5, 40))
    n = len(pairs)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    plain = batch(hip, NUC, GAPS, pairs, size=(32, 256))
    sized = hip.SizedBatchAligner(NUC, GAPS, 0, 0, *args, percent=(0.05, 0.2))
    multi = hip.MultiBatchAligner(NUC, GAPS, (32, 256), 0, 0, *args, devices=[0, 0])
    assert len(sized.classes()) > 1
    rng = np.random.default_rng(7)
    for what, x in ((hip.EXACT_GLOBAL, -1), (hip.EXACT_EXTEND, 20)):
        rec, runs, off = plain.exact_cigars(what, x)
        full = split(runs, off)
        want_rec, want_runs = helper(pairs, NUC, GAPS, "global" if what == hip.EXACT_GLOBAL else "extend", x)
        assert records(rec) == want_rec and full == want_runs
        for which in (rng.permutation(n), rng.integers(0, n, 2 * n), np.array([n - 1, n - 1, 0, n - 1]), np.zeros(0, np.uint32)):
            for bt in (plain, sized, multi):
                r2, runs2, off2 = bt.exact_cigars(what, x, which)
                assert records(r2) == [records(rec)[int(p)] for p in which]
                assert split(runs2, off2) == [full[int(p)] for p in which]
        for bt in (sized, multi):
            r2, runs2, off2 = bt.exact_cigars(what, x)
            assert records(r2) == records(rec) and np.array_equal(runs2, runs) and np.array_equal(off2, off)
    with pytest.raises(RuntimeError, match=rf"\b{n + 3}\b.*out of range"):
        plain.exact_cigars(hip.EXACT_GLOBAL, -1, [0, n + 3])
    # the two-call pattern by hand: sizes only; an undersized buffer is refused with the count needed and the offsets are still filled; the
    # repeated call gives the same bytes and computes nothing (the time of the last computing call stays)
    L = hip.lib()
    rec, runs, off = plain.exact_cigars(hip.EXACT_GLOBAL, -1)
    ms0 = plain.exact_cigars_ms()
    assert ms0[0] > 0 and ms0[1] == int(((pairs.q_len.astype(np.int64) + 1) * (pairs.r_len.astype(np.int64) + 1)).sum())
    r2, off2 = np.zeros(n, hip.EXACT_DTYPE), np.zeros(n + 1, np.uint64)
    assert L.ba_batch_exact_cigars(plain._h, 0, -1, None, 0, r2.ctypes.data, off2.ctypes.data, None, 0) == 0
    assert np.array_equal(off2, off) and records({k: r2[k] for k in FIELDS}) == records(rec)
    small, off3 = np.zeros(len(runs) - 1, np.uint32), np.zeros(n + 1, np.uint64)
    assert L.ba_batch_exact_cigars(plain._h, 0, -1, None, 0, r2.ctypes.data, off3.ctypes.data, small.ctypes.data, small.size) != 0
    assert f"the request has {len(runs)}" in hip.last_error() and np.array_equal(off3, off)
    again = np.zeros(len(runs), np.uint32)
    assert L.ba_batch_exact_cigars(plain._h, 0, -1, None, 0, r2.ctypes.data, off3.ctypes.data, again.ctypes.data, again.size) == 0
    assert again.tobytes() == runs.tobytes() and plain.exact_cigars_ms() == ms0
    assert L.ba_batch_exact_cigars(plain._h, 0, -1, None, 0, r2.ctypes.data, None, None, 0) != 0 and "run_off" in hip.last_error()
    # after a reload the kept request is not answered from the device: the new pairs' paths
    other = synth.make_pairs(50, (0, 300), (0, 30), 20, synth.DNA, seed=331)
    plain.reload(other.pool, other.q_off, other.q_len, other.r_off, other.r_len)
    rec, runs, off = plain.exact_cigars(hip.EXACT_GLOBAL, -1)
    want_rec, want_runs = helper(other, NUC, GAPS, "global", -1)
    assert records(rec) == want_rec and split(runs, off) == want_runs
    for x in (plain, sized, multi):
        x.close()


# ---------------------------------------------------------------- 5. BA_CIGAR_EQ
def collapse(runs):
    out = []
    for x in runs:
        op, n = (1 if (x & 15) in (2, 3) else x & 15), x >> 4
        if out and out[-1][0] == op:
            out[-1][1] += n
        else:
            out.append([op, n])
    return [(n << 4) | op for op, n in out]


@pytest.mark.parametrize("kind", ["nuc", "bytes"])
def test_cigar_eq(hip, kind):
    m, gaps, _a = kinds()[kind]
    pairs = length_pairs(kind)
    beq, bm = batch(hip, m, gaps, pairs, mode=hip.CIGAR_EQ), batch(hip, m, gaps, pairs)
    rec_eq, runs_eq, off_eq = beq.exact_cigars(hip.EXACT_GLOBAL)
    rec_m, runs_m, off_m = bm.exact_cigars(hip.EXACT_GLOBAL)
    beq.close(); bm.close()
    eq, mm = split(runs_eq, off_eq), split(runs_m, off_m)
    assert records(rec_eq) == records(rec_m)
    assert all({x & 15 for x in c} <= {2, 3, 4, 5} for c in eq) and all({x & 15 for x in c} <= {1, 4, 5} for c in mm)
    assert any(3 in {x & 15 for x in c} for c in eq)
    assert [collapse(c) for c in eq] == mm
    assert eq == helper(pairs, m, gaps, "global", -1, eq=True)[1]


# ---------------------------------------------------------------- 6. refusals
def test_refusals(hip):
    pairs = synth.make_pairs(8, 100, 5, 10, synth.AMINO, seed=540)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    m = S.static_matrix("BLOSUM62")
    profiles = [S.AAProfile.from_bytes(pairs.reference(p), 64, 2, -1, -5, 0, -5, -1) for p in range(len(pairs))]
    pb = hip.ProfileBatchAligner(profiles, (32, 64), 0, 0, pairs.pool, pairs.q_off, pairs.q_len)
    with pytest.raises(RuntimeError, match="profile batches are not supported"):
        pb.exact_cigars()
    pb.close()
    for mode in (hip.LOCAL_START, hip.FREE_QUERY_END_GAPS, hip.FREE_QUERY_START_GAPS):
        b = hip.BatchAligner(m, (-11, -1), (128, 128), 0, mode, *args)
        with pytest.raises(RuntimeError, match="BA_LOCAL_START or BA_FREE_QUERY"):
            b.exact_cigars()
        b.close()
    b = hip.BatchAligner(m, (-11, -1), (32, 128), 0, 0, *args)
    with pytest.raises(RuntimeError, match="unknown quantity 7"):
        b.exact_cigars(7)
    b.launch()
    with pytest.raises(RuntimeError, match="in flight"):
        b.exact_cigars()
    b.wait()
    rec, runs, off = b.exact_cigars()
    assert len(off) == len(pairs) + 1 and int(off[-1]) == len(runs) > 0
    b.close()
    ss = seed_set()
    eb = hip.ExtendBatchAligner(NUC, GAPS, (32, 256), 60, hip.X_DROP, *ss.args(), strand=ss.strand)
    assert not hasattr(eb, "exact_cigars") and not hasattr(hip.lib(), "ba_extend_batch_exact_cigars")
    eb.close()


# ---------------------------------------------------------------- 7. the use case: rescue what the block range got wrong
def test_rescue_of_wrong_pairs(hip):
    """A long insertion in the query takes the block path off the optimum when the blocks are too small to span it. The pairs are chosen
    on the CPU (by construction: every other pair carries a 200-letter indel); accuracy() must report some of them below the optimum, and
    their exact paths score higher than the block paths and rescore to exact()."""
    rng = np.random.default_rng(340)
    lists = []
    for n in range(32):
        base = synth.rand_str(rng, 900, synth.DNA)
        q = synth.mutate(rng, base, 20, synth.DNA)
        if n % 2:
            q = np.concatenate([q[:400], synth.rand_str(rng, 200, synth.DNA), q[400:]])
        lists.append((q.tobytes(), base.tobytes()))
    pairs = synth.PairSet.from_lists(lists)
    which = np.arange(1, 32, 2)
    b = batch(hip, NUC, GAPS, pairs, size=(32, 64), mode=hip.TRACE)
    b.run()
    res = b.results()
    acc = b.accuracy(which=which)
    assert acc["below"] > 0 and acc["above"] == 0
    ex = b.exact(which=which)
    rec, runs, off = b.exact_cigars(which=which)
    b.close()
    assert records(rec) == records(ex)
    got = split(runs, off)
    wrong = [k for k, p in enumerate(which) if int(res["score"][p]) < int(ex["score"][k])]
    assert len(wrong) == acc["below"]
    for k, p in enumerate(which):
        check_cigar(got[k], pairs.query(int(p)), pairs.reference(int(p)), NUC, GAPS, int(ex["score"][k]), int(ex["query_idx"][k]), int(ex["reference_idx"][k]), what=int(p))
    assert all(int(res["score"][which[k]]) < int(rec["score"][k]) for k in wrong)      # the block path scores lower than the exact path
