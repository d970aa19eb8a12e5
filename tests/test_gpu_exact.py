"""Exact full-matrix scores on the MI355X (ba_*_exact): every record of every pair against the numpy DP of tests/exact_dp.py and
tests/gotoh.py, the upper bound on the block heuristic through every fill kernel, pair selection, sized / multi / extension batches,
the refusals, and the accuracy summary. Every assertion covers every pair of its inputs."""
import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import exact_dp, gotoh
from tests.test_gpu_extend import SeedSet

pytestmark = pytest.mark.gpu

NUC = S.NucMatrix.new_simple(2, -3)
BYTES = S.ByteMatrix.new_simple(3, -2)
GAPS = (-5, -1)
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 500, 1500, 2000)
FIELDS = ("score", "query_idx", "reference_idx", "rows")
AMINO = synth.AMINO
BYTE_ALPHABET = np.arange(250, 256, dtype=np.uint8)


def kinds():
    return {"nuc": (NUC, GAPS, synth.DNA), "aa": (S.static_matrix("BLOSUM62"), (-11, -1), AMINO), "bytes": (BYTES, (-4, -2), BYTE_ALPHABET)}


def related(rng, nq, nr, alphabet, lower=False):
    """A pair of the given lengths that shares a mutated common part, so that the best path is not trivial."""
    base = synth.rand_str(rng, max(nq, nr), alphabet)
    q = synth.mutate(rng, base, max(nq, nr) // 12, alphabet)
    q = np.concatenate([q, synth.rand_str(rng, nq, alphabet)])[:nq]
    r = base[:nr]
    qb, rb = q.tobytes(), r.tobytes()
    return (qb.lower(), rb) if lower else (qb, rb)


def length_pairs(kind, count, seed):
    """Pairs whose two lengths are drawn independently from LENGTHS: every ordered combination first, `count` of them in a seeded order."""
    rng = np.random.default_rng(seed)
    combos = [(a, b) for a in LENGTHS for b in LENGTHS]
    order = rng.permutation(len(combos))[:count]
    _m, _g, alphabet = kinds()[kind]
    lists = [related(rng, *combos[k], alphabet, lower=(kind != "bytes" and n % 4 == 0)) for n, k in enumerate(order)]
    assert any(len(q) > len(r) for q, r in lists) and any(len(q) < len(r) for q, r in lists)
    return synth.PairSet.from_lists(lists)


def batch(hip, m, gaps, pairs, size=(32, 128), x_drop=0, mode=0):
    return hip.BatchAligner(m, gaps, size, x_drop, mode, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)


def records(ex):
    return [tuple(int(ex[k][p]) for k in FIELDS) for p in range(len(ex["score"]))]


# ---------------------------------------------------------------- 1. GLOBAL against the numpy DP
@pytest.mark.parametrize("kind,count", [("nuc", 169), ("aa", 60), ("bytes", 60)])
def test_global_equals_gotoh(hip, kind, count):
    m, gaps, _a = kinds()[kind]
    pairs = length_pairs(kind, count, seed=100 + count)
    b = batch(hip, m, gaps, pairs)
    ex = b.exact(hip.EXACT_GLOBAL)
    b.close()
    want = [(gotoh.global_score(pairs.query(p), pairs.reference(p), m, gaps), int(pairs.q_len[p]), int(pairs.r_len[p]), int(pairs.q_len[p]) + 1)
            for p in range(len(pairs))]
    assert records(ex) == want


# ---------------------------------------------------------------- 2. EXTEND without X-drop
@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_extend_equals_helper(hip, kind):
    m, gaps, _a = kinds()[kind]
    pairs = length_pairs(kind, 48, seed=200)
    b = batch(hip, m, gaps, pairs, x_drop=30, mode=hip.X_DROP)
    ex = b.exact(hip.EXACT_EXTEND, -1)
    assert records(b.exact()) == records(ex)          # an X-drop batch: EXTEND is the default
    b.close()
    want = [exact_dp.exact_extend(pairs.query(p), pairs.reference(p), m, gaps, -1) for p in range(len(pairs))]
    assert records(ex) == want


# ---------------------------------------------------------------- 3. EXTEND with X-drop
def xdrop_pairs(seed=31):
    """A related prefix followed by an unrelated suffix. A third of the pairs has no edits and no suffix (no row ever drops), a third a long
    suffix (every threshold stops inside it), a third a short one."""
    rng = np.random.default_rng(seed)
    lists = []
    for n in range(48):
        pre = synth.rand_str(rng, int(rng.integers(40, 400)), synth.DNA)
        if n % 3 == 0:
            q, r = pre, pre
        else:
            tail = int(rng.integers(250, 600)) if n % 3 == 1 else int(rng.integers(4, 30))
            q = np.concatenate([synth.mutate(rng, pre, len(pre) // 25, synth.DNA), synth.rand_str(rng, tail, synth.DNA)])
            r = np.concatenate([pre, synth.rand_str(rng, tail + int(rng.integers(0, 40)), synth.DNA)])
        lists.append((q.tobytes(), r.tobytes()))
    return synth.PairSet.from_lists(lists)


@pytest.mark.parametrize("x_drop", [0, 20, 50])
def test_extend_x_drop_equals_helper(hip, x_drop):
    pairs = xdrop_pairs()
    want = [exact_dp.exact_extend(pairs.query(p), pairs.reference(p), NUC, GAPS, x_drop) for p in range(len(pairs))]
    early = sum(w[3] < int(pairs.q_len[p]) + 1 for p, w in enumerate(want))
    assert early * 4 >= len(pairs) and (len(pairs) - early) * 4 >= len(pairs), early      # both branches are exercised
    b = batch(hip, NUC, GAPS, pairs, x_drop=x_drop, mode=hip.X_DROP)
    ex = b.exact(hip.EXACT_EXTEND, x_drop)
    b.close()
    assert records(ex) == want


# ---------------------------------------------------------------- 4. upper bound on the heuristic
ROUTES = {
    # size, development switch, kernel, matrix, gaps, pairs
    "k_small_dna": ((32, 256), "BA_FORCE_SMALL", "k_small", "nuc", lambda: synth.make_pairs(200, (200, 1500), (0, 120), 40, synth.DNA, seed=501, indels=2, indel_len=(10, 80))),
    "k_small_protein": ((32, 256), "BA_FORCE_SMALL", "k_small", "aa", lambda: synth.make_pairs(200, (50, 800), (0, 80), 20, AMINO, seed=502, indels=1, indel_len=(5, 40))),
    "k_multi_10k": ((128, 1024), "BA_FORCE_MULTI", "k_multi", "nuc", lambda: synth.make_pairs(48, 10000, 1000, 500, synth.DNA, seed=503)),
    "k_align": ((32, 256), None, "k_align", "nuc", lambda: synth.make_pairs(200, (0, 1500), (0, 120), 40, synth.DNA, seed=504, indels=2, indel_len=(10, 80))),
}


@pytest.mark.parametrize("x_drop_mode", [False, True])
@pytest.mark.parametrize("trace", [False, True])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_exact_bounds_the_heuristic(devlib, monkeypatch, route, trace, x_drop_mode):
    hip = devlib
    size, switch, kernel, kind, make = ROUTES[route]
    if switch:
        monkeypatch.setenv(switch, "1")
    m, gaps, _a = kinds()[kind]
    pairs = make()
    mode = (hip.TRACE if trace else 0) | (hip.X_DROP if x_drop_mode else 0)
    b = batch(hip, m, gaps, pairs, size=size, x_drop=100 if x_drop_mode else 0, mode=mode)
    assert b.info()["kernel"] == kernel
    b.run()
    res = b.results()
    ex = b.exact(x_drop=-1)
    again = b.results()
    b.close()
    assert not res["status"].any()
    assert all(np.array_equal(res[k], again[k]) for k in res)          # the exact call leaves the run's results alone
    assert (ex["score"] >= res["score"]).all(), np.flatnonzero(ex["score"] < res["score"])
    assert (ex["rows"] == pairs.q_len + 1).all()


@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_one_block_over_the_matrix_gives_equality(hip, kind):
    m, gaps, alphabet = kinds()[kind]
    pairs = synth.make_pairs(64, (0, 200), (0, 30), 10, alphabet, seed=510, indels=1, indel_len=(3, 20))
    assert int(max(pairs.q_len.max(), pairs.r_len.max())) < 256
    for trace in (0, hip.TRACE):
        b = batch(hip, m, gaps, pairs, size=(256, 256), mode=trace)
        b.run()
        res = b.results()
        ex = b.exact()                                                 # a global batch: GLOBAL is the default
        b.close()
        assert np.array_equal(ex["score"], res["score"])
        assert np.array_equal(ex["query_idx"], res["query_idx"]) and np.array_equal(ex["reference_idx"], res["reference_idx"])


# ---------------------------------------------------------------- 5. pair selection
def test_pair_selection(hip):
    pairs = synth.make_pairs(40, (0, 400), (0, 40), 20, synth.DNA, seed=520)
    n = len(pairs)
    b = batch(hip, NUC, GAPS, pairs)
    rng = np.random.default_rng(5)
    for what, x in ((hip.EXACT_GLOBAL, -1), (hip.EXACT_EXTEND, -1), (hip.EXACT_EXTEND, 20)):
        full = records(b.exact(what, x))
        assert records(b.exact(what, x, np.arange(n))) == full
        for which in (rng.permutation(n), rng.permutation(n)[:7], rng.integers(0, n, 3 * n), np.array([n - 1, n - 1, 0, n - 1])):
            assert records(b.exact(what, x, which)) == [full[int(p)] for p in which]
        assert records(b.exact(what, x, np.zeros(0, np.uint32))) == []
    with pytest.raises(RuntimeError, match=rf"\b{n + 3}\b.*out of range"):
        b.exact(hip.EXACT_GLOBAL, -1, [0, 1, n + 3])
    b.close()


# ---------------------------------------------------------------- 6. sized and multi batches
def test_sized_and_multi_batches(hip):
    pairs = synth.make_pairs(60, (0, 900), (0, 60), 30, synth.DNA, seed=530, indels=1, indel_len=(5, 60))
    other = synth.make_pairs(50, (0, 700), (0, 60), 30, synth.DNA, seed=531)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    plain = batch(hip, NUC, GAPS, pairs, size=(32, 256))
    sized = hip.SizedBatchAligner(NUC, GAPS, 0, 0, *args, percent=(0.05, 0.2))
    multi = hip.MultiBatchAligner(NUC, GAPS, (32, 256), 0, 0, *args, devices=[0, 0])
    assert len(sized.classes()) > 1
    which = np.random.default_rng(6).integers(0, len(pairs), 90)
    for what, x in ((hip.EXACT_GLOBAL, -1), (hip.EXACT_EXTEND, -1), (hip.EXACT_EXTEND, 20)):
        want, want_sel = records(plain.exact(what, x)), records(plain.exact(what, x, which))
        for other_batch in (sized, multi):
            assert records(other_batch.exact(what, x)) == want
            assert records(other_batch.exact(what, x, which)) == want_sel
    with pytest.raises(RuntimeError, match="out of range"):
        sized.exact(which=[len(pairs)])
    plain.reload(other.pool, other.q_off, other.q_len, other.r_off, other.r_len)
    got = records(plain.exact(hip.EXACT_GLOBAL))
    assert got == [(gotoh.global_score(other.query(p), other.reference(p), NUC, GAPS), int(other.q_len[p]), int(other.r_len[p]), int(other.q_len[p]) + 1)
                   for p in range(len(other))]
    for x in (plain, sized, multi):
        x.close()


# ---------------------------------------------------------------- 7. extension batches
def seed_set(seed=41):
    """Seeds inside related sequences, both strands; seeds 0 .. 3 have an empty left side, an empty right side, both, and an empty query side."""
    rng = np.random.default_rng(seed)
    seqs, q_idx, r_idx, q_seed, r_seed, seed_len, strand = [], [], [], [], [], [], []
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    for n in range(28):
        r = synth.rand_str(rng, int(rng.integers(150, 700)), synth.DNA)
        L = int(rng.integers(8, 24))
        t = int(rng.integers(0, len(r) - L))
        left = synth.mutate(rng, r[:t], t // 15, synth.DNA)
        right = synth.mutate(rng, r[t + L:], (len(r) - t - L) // 15, synth.DNA)
        if n == 0:
            left, r, t = left[:0], r[t:], 0
        if n == 1:
            right, r = right[:0], r[:t + L]
        if n == 2:
            left, right, r, t = left[:0], right[:0], r[t:t + L], 0
        if n == 3:
            left = left[:0]                      # the query starts at the seed, the reference does not: no left side either
        q = np.concatenate([left, r[t:t + L], right]).tobytes()
        st = int(n % 3 == 2 and n > 3)
        seqs += [q.translate(comp)[::-1] if st else q, r.tobytes()]
        q_idx.append(2 * n); r_idx.append(2 * n + 1); q_seed.append(len(left)); r_seed.append(t); seed_len.append(L); strand.append(st)
    return SeedSet(seqs, q_idx, r_idx, q_seed, r_seed, seed_len, strand)


@pytest.mark.parametrize("x_drop", [-1, 30])
def test_extension_batches(hip, x_drop):
    ss = seed_set()
    assert ss.strand.any()
    eb = hip.ExtendBatchAligner(NUC, GAPS, (32, 256), 60, hip.X_DROP, *ss.args(), strand=ss.strand)
    ex = eb.exact(x_drop)                         # before any run
    eb.run()
    res = eb.results()
    zero = (0, 0, 0, 0)
    empties = 0
    for p in range(len(ss)):
        q, r = ss.q(p), ss.r(p)
        s, t, L = int(ss.q_seed[p]), int(ss.r_seed[p]), int(ss.seed_len[p])
        sides = ((q[:s][::-1], r[:t][::-1]), (q[s + L:], r[t + L:]))
        want = [exact_dp.exact_extend(a, b, NUC, GAPS, x_drop) if a and b else zero for a, b in sides]
        empties += want.count(zero)
        got = [tuple(int(ex[w][k][p]) for k in FIELDS) for w in ("left", "right")]
        assert got == want, p
        seed_score = sum(NUC.get(a, b) for a, b in zip(q[s:s + L], r[t:t + L]))
        assert int(ex["score"][p]) == want[0][0] + seed_score + want[1][0], p
    assert empties >= 5
    assert not res["status"].any()
    if x_drop < 0:
        assert (ex["score"] >= res["score"]).all()
        acc = eb.accuracy()
        assert acc == hip.accuracy_summary(res["score"], ex["score"], status=res["status"]) and acc["above"] == 0 and acc["n"] == len(ss)
    which = np.array([5, 0, 5, 27, 2])
    sel = eb.exact(x_drop, which)
    assert np.array_equal(sel["score"], ex["score"][which])
    assert all(np.array_equal(sel[w][k], ex[w][k][which]) for w in ("left", "right") for k in FIELDS)
    with pytest.raises(RuntimeError, match="out of range"):
        eb.exact(x_drop, [len(ss)])
    eb.close()


# ---------------------------------------------------------------- 8. refusals
def test_refusals(hip):
    pairs = synth.make_pairs(8, 100, 5, 10, AMINO, seed=540)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    m = S.static_matrix("BLOSUM62")
    profiles = [S.AAProfile.from_bytes(pairs.reference(p), 64, 2, -1, -5, 0, -5, -1) for p in range(len(pairs))]
    pb = hip.ProfileBatchAligner(profiles, (32, 64), 0, 0, pairs.pool, pairs.q_off, pairs.q_len)
    with pytest.raises(RuntimeError, match="profile"):
        pb.exact()
    pb.close()
    for mode in (hip.LOCAL_START, hip.FREE_QUERY_END_GAPS, hip.FREE_QUERY_START_GAPS):
        b = hip.BatchAligner(m, (-11, -1), (128, 128), 0, mode, *args)     # (FREE_QUERY_END_GAPS: the min block must exceed the query)
        with pytest.raises(RuntimeError, match="LOCAL_START"):
            b.exact()
        b.close()
    b = hip.BatchAligner(m, (-11, -1), (32, 128), 0, 0, *args)
    with pytest.raises(RuntimeError, match="unknown quantity 7"):
        b.exact(7)
    assert hip.lib().ba_batch_exact(b._h, 0, -1, None, 0, None) != 0 and "out" in hip.last_error()
    b.launch()
    with pytest.raises(RuntimeError, match="in flight"):
        b.exact()
    b.wait()
    assert len(b.exact()["score"]) == len(pairs)
    b.close()
    # a pair past the int32 guard: the planning check on synthetic lengths, nothing is allocated
    with pytest.raises(RuntimeError, match=r"pair 1 .*too long"):
        hip.exact_check_lengths([100, 1 << 23], [100, 1])


# ---------------------------------------------------------------- 9. accuracy and timing
def test_accuracy_and_timing(hip):
    pairs = synth.make_pairs(300, (100, 1200), (0, 150), 40, synth.DNA, seed=550, indels=3, indel_len=(20, 120))
    for mode, x_drop in ((0, 0), (hip.X_DROP, 40)):
        b = batch(hip, NUC, GAPS, pairs, size=(32, 64), x_drop=x_drop, mode=mode)
        b.run()
        res = b.results()
        ex = b.exact(x_drop=-1)
        ms, cells = b.exact_ms()
        assert ms > 0 and cells == int((ex["rows"].astype(np.int64) * (pairs.r_len.astype(np.int64) + 1)).sum())
        acc = b.accuracy()
        assert acc == hip.accuracy_summary(res["score"], ex, res["query_idx"], res["reference_idx"], res["status"])
        assert acc["n"] == acc["compared"] == len(pairs) and acc["above"] == 0 and acc["wrong"] == acc["below"]
        which = np.array([7, 3, 3, 250])
        sub = b.accuracy(which=which)
        ms2, cells2 = b.exact_ms()
        assert sub["n"] == 4 and cells2 == int((ex["rows"][which].astype(np.int64) * (pairs.r_len[which].astype(np.int64) + 1)).sum())
        b.close()
