"""Exact full-matrix scores in the batch's own mode on the MI355X (ba_*_exact with BA_EXACT_OWN_MODE): every record of LOCAL_START,
FREE_QUERY_START_GAPS, FREE_QUERY_END_GAPS and profile batches against the numpy models of tests/exact_modes_dp.py, the tie to a run with one
block over the matrix, the inert flag on plain batches, pair selection, sized / multi batches, accuracy(own_mode=True) and the refusals.
Every call passes the flag: on a library without it each test fails with "unknown quantity". Every assertion covers every pair."""
import functools

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import exact_modes_dp as M
from tests.test_gotoh import AA20
from tests.test_gpu_exact import batch, kinds, records, related
from tests.test_gpu_extend import SeedSet

pytestmark = pytest.mark.gpu

# the band hand-over through the row buffer (64 / 65, 128 / 129), a short last band, the 64-column chunk reload and a chunk that ends
# inside the matrix; the profile sweep owns row 0, so its bands turn over one query row earlier (63 / 64)
Q_LENGTHS = (1, 15, 63, 64, 65, 128, 129)
R_LENGTHS = (1, 63, 64, 65, 127, 200)
RANDOM_SHAPES = ((255, 300), (200, 31), (97, 256), (3, 290), (250, 129))      # (every query below 256: FREE_QUERY_END_GAPS' minimum block)
X_DROPS = (-1, 0, 30)
AA = np.frombuffer(AA20, np.uint8)


def shapes():
    return [(a, b) for a in Q_LENGTHS for b in R_LENGTHS] + list(RANDOM_SHAPES)


@functools.lru_cache(maxsize=None)
def seq_pairs(kind):
    rng = np.random.default_rng({"nuc": 81, "aa": 82, "bytes": 83}[kind])
    _m, _g, alphabet = kinds()[kind]
    return synth.PairSet.from_lists([related(rng, nq, nr, alphabet, lower=(kind != "bytes" and n % 4 == 0)) for n, (nq, nr) in enumerate(shapes())])


SEQ_MODES = {
    # name -> (mode bits, model's start rule, FREE_QUERY_END_GAPS)
    "local_start": (lambda H: H.LOCAL_START, dict(local_start=True), False),
    "free_query_start_gaps": (lambda H: H.FREE_QUERY_START_GAPS, dict(free_query_start=True), False),
    "free_query_end_gaps": (lambda H: H.FREE_QUERY_END_GAPS, {}, True),
    "local_start+free_query_end_gaps": (lambda H: H.LOCAL_START | H.FREE_QUERY_END_GAPS, dict(local_start=True), True),
    "free_query_start_gaps+free_query_end_gaps": (lambda H: H.FREE_QUERY_START_GAPS | H.FREE_QUERY_END_GAPS, dict(free_query_start=True), True),
}


@functools.lru_cache(maxsize=None)
def seq_matrices(kind, mode):
    """The model's H of every pair of seq_pairs(kind) under the mode's start rule; computed once, shared, never changed."""
    m, gaps, _a = kinds()[kind]
    pairs = seq_pairs(kind)
    return tuple(M.full_matrix_mode(pairs.query(p), pairs.reference(p), m, gaps, **SEQ_MODES[mode][1]) for p in range(len(pairs)))


def model_records(Hs, what, x_drop, free_end):
    return [M.own_mode(H, what, x_drop, free_end) for H in Hs]


# ---------------------------------------------------------------- 1. sequence modes against the model
@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
@pytest.mark.parametrize("mode", ["local_start", "free_query_start_gaps", "free_query_end_gaps"])
def test_sequence_modes_equal_the_model(hip, kind, mode):
    sequence_mode_case(hip, kind, mode)


@pytest.mark.parametrize("mode", ["local_start+free_query_end_gaps", "free_query_start_gaps+free_query_end_gaps"])
def test_start_and_end_rules_combine(hip, mode):
    sequence_mode_case(hip, "nuc", mode)


def sequence_mode_case(hip, kind, mode):
    m, gaps, _a = kinds()[kind]
    bits, _kw, free_end = SEQ_MODES[mode]
    pairs = seq_pairs(kind)
    Hs = seq_matrices(kind, mode)
    b = batch(hip, m, gaps, pairs, size=(256, 256), mode=bits(hip))      # (FREE_QUERY_END_GAPS: the minimum block exceeds every query)
    got_global = records(b.exact(hip.EXACT_GLOBAL, own_mode=True))
    assert records(b.exact(own_mode=True)) == got_global                   # no X-drop: GLOBAL is the default
    assert records(b.exact(hip.EXACT_GLOBAL | hip.EXACT_OWN_MODE)) == got_global
    got_extend = {x: records(b.exact(hip.EXACT_EXTEND, x, own_mode=True)) for x in X_DROPS}
    b.close()
    assert got_global == model_records(Hs, "global", -1, free_end)
    for x in X_DROPS:
        assert got_extend[x] == model_records(Hs, "extend", x, free_end), x
    if free_end:
        assert any(r[2] < int(pairs.r_len[p]) for p, r in enumerate(got_global))      # the last-row maximum is not always the corner
    assert any(r[3] < int(pairs.q_len[p]) + 1 for p, r in enumerate(got_extend[0]))   # the X-drop rule stops somewhere


# ---------------------------------------------------------------- 2. profiles against the model
def make_profile(rng, nq, nr, B, ge, form):
    """A PSSM of nr positions over a random consensus and a query of nq residues related to it. form: "uniform" gap costs (close 0),
    position-"specific" ones (open_C, open_R < 0, close_C in -4 .. 0), or "tail": specific, the last positions never set (-128)."""
    cons = AA[rng.integers(0, 20, nr)]
    p = S.AAProfile(nr, B, ge)
    have = nr - min(5, nr // 3) if form == "tail" else nr
    for i in range(have):
        for a in AA:
            p.set(i + 1, int(a), S.BLOSUM62.get(int(cons[i]), int(a)))
    go = int(rng.integers(-12, -4))
    for i in range(have + 1):
        if form == "uniform":
            p.set_gap_open_C(i, go); p.set_gap_close_C(i, 0); p.set_gap_open_R(i, go)
        else:
            p.set_gap_open_C(i, int(rng.integers(-14, -3))); p.set_gap_open_R(i, int(rng.integers(-14, -3))); p.set_gap_close_C(i, int(rng.integers(-4, 1)))
    q = synth.mutate(rng, cons, nr // 8, AA)
    q = np.concatenate([q, synth.rand_str(rng, nq, AA)])[:nq].astype(np.uint8).tobytes()
    return (q.lower() if nq % 2 else q), p


@functools.lru_cache(maxsize=None)
def profile_set(ge, B=512):
    """(queries as a PairSet, profiles, the model's H per pair) over every shape, the three forms in turn."""
    rng = np.random.default_rng(90 - ge)
    cases = [make_profile(rng, nq, nr, B, ge, ("specific", "uniform", "tail")[n % 3]) for n, (nq, nr) in enumerate(shapes())]
    pairs = synth.PairSet.from_lists([(q, b"A") for q, _p in cases])
    profiles = [p for _q, p in cases]
    assert any(p.pos_gap_close_C[1] != 0 for p in profiles) and any(p.pos_aa[p.str_len, 0] == -128 for p in profiles)
    return pairs, profiles, tuple(M.full_matrix_profile(q, p) for q, p in cases)


def profile_batch(hip, pairs, profiles, size=(512, 512), x_drop=0, mode=0):
    return hip.ProfileBatchAligner(profiles, size, x_drop, mode, pairs.pool, pairs.q_off, pairs.q_len)


@pytest.mark.parametrize("ge", [-1, -2])
def test_profiles_equal_the_model(hip, ge):
    pairs, profiles, Hs = profile_set(ge)
    b = profile_batch(hip, pairs, profiles)
    got_global = records(b.exact(hip.EXACT_GLOBAL, own_mode=True))
    got_extend = {x: records(b.exact(hip.EXACT_EXTEND, x, own_mode=True)) for x in X_DROPS}
    b.close()
    assert got_global == model_records(Hs, "global", -1, False)
    for x in X_DROPS:
        assert got_extend[x] == model_records(Hs, "extend", x, False), x
    assert any(r[3] < len(H) for r, H in zip(got_extend[0], Hs))


# ---------------------------------------------------------------- 3. the tie to a run with one block over the matrix
@pytest.mark.parametrize("mode", ["local_start", "free_query_start_gaps"])
def test_one_block_run_equals_own_mode_global(hip, mode):
    m, gaps, _a = kinds()["nuc"]
    pairs = seq_pairs("nuc")
    bits = SEQ_MODES[mode][0](hip)
    b = batch(hip, m, gaps, pairs, size=(512, 512), mode=bits)
    b.run()
    res = b.results()
    ex = b.exact(hip.EXACT_GLOBAL, own_mode=True)
    b.close()
    assert not res["status"].any()
    assert np.array_equal(res["score"], ex["score"])
    assert np.array_equal(res["query_idx"], ex["query_idx"]) and np.array_equal(res["reference_idx"], ex["reference_idx"])
    bx = batch(hip, m, gaps, pairs, size=(512, 512), x_drop=40, mode=bits | hip.X_DROP)
    bx.run()
    resx = bx.results()
    exx = bx.exact(x_drop=-1, own_mode=True)                               # an X-drop batch: EXTEND is the default
    bx.close()
    assert not resx["status"].any()
    assert (resx["score"] <= exx["score"]).all(), np.flatnonzero(resx["score"] > exx["score"])


@pytest.mark.parametrize("ge", [-1, -2])
def test_one_block_profile_run_equals_own_mode_global(hip, ge):
    pairs, profiles, _Hs = profile_set(ge)
    b = profile_batch(hip, pairs, profiles)
    b.run()
    res = b.results()
    ex = b.exact(own_mode=True)
    b.close()
    assert not res["status"].any()
    assert np.array_equal(res["score"], ex["score"])
    bx = profile_batch(hip, pairs, profiles, x_drop=40, mode=hip.X_DROP)
    bx.run()
    resx = bx.results()
    exx = bx.exact(x_drop=-1, own_mode=True)
    bx.close()
    assert not resx["status"].any()
    assert (resx["score"] <= exx["score"]).all(), np.flatnonzero(resx["score"] > exx["score"])


def test_one_block_free_query_end_gaps_short_queries(hip):
    """|q| < 16: the run reports max(exact, 0)."""
    rng = np.random.default_rng(84)
    lists = []
    for n in range(40):
        r = synth.rand_str(rng, int(rng.integers(1, 200)), synth.DNA)
        nq = int(rng.integers(1, 16))
        a = int(rng.integers(0, len(r)))
        q = synth.mutate(rng, r[a:a + nq], 1, synth.DNA) if n % 2 and len(r[a:a + nq]) else synth.rand_str(rng, nq, synth.DNA)
        lists.append((q.tobytes(), r.tobytes()))
    pairs = synth.PairSet.from_lists(lists)
    m = S.NucMatrix.new_simple(1, -9)
    b = batch(hip, m, (-7, -2), pairs, size=(256, 256), mode=hip.FREE_QUERY_END_GAPS)
    b.run()
    res = b.results()
    ex = b.exact(hip.EXACT_GLOBAL, own_mode=True)
    b.close()
    assert not res["status"].any() and (ex["score"] < 0).any() and (ex["score"] > 0).any()
    assert np.array_equal(res["score"], np.maximum(ex["score"], 0))
    want = [M.own_mode(M.full_matrix_mode(q, r, m, (-7, -2)), "global", free_query_end=True) for q, r in lists]
    assert records(ex) == want


# ---------------------------------------------------------------- 4. the flag is inert on a plain batch
@pytest.mark.parametrize("kind", ["nuc", "bytes"])
def test_flag_is_inert_on_plain_batches(hip, kind):
    m, gaps, _a = kinds()[kind]
    pairs = seq_pairs(kind)
    b = batch(hip, m, gaps, pairs)
    for what, x in ((hip.EXACT_GLOBAL, -1), (hip.EXACT_EXTEND, -1), (hip.EXACT_EXTEND, 30)):
        assert records(b.exact(what | hip.EXACT_OWN_MODE, x)) == records(b.exact(what, x))
        assert records(b.exact(what, x, own_mode=True)) == records(b.exact(what, x))
    rec, runs, off = b.exact_cigars(hip.EXACT_GLOBAL | hip.EXACT_OWN_MODE)      # ... and for the paths of a plain batch
    rec0, runs0, off0 = b.exact_cigars(hip.EXACT_GLOBAL)
    b.close()
    assert records(rec) == records(rec0) and np.array_equal(runs, runs0) and np.array_equal(off, off0)


# ---------------------------------------------------------------- 5. pair selection on a profile batch
def test_which_selection_on_a_profile_batch(hip):
    pairs, profiles, Hs = profile_set(-1)
    n = len(pairs)
    b = profile_batch(hip, pairs, profiles)
    rng = np.random.default_rng(85)
    for what, name, x in ((hip.EXACT_GLOBAL, "global", -1), (hip.EXACT_EXTEND, "extend", 30)):
        full = model_records(Hs, name, x, False)
        for which in (rng.permutation(n), rng.permutation(n)[:7], rng.integers(0, n, 2 * n), np.array([n - 1, n - 1, 0, n - 1])):
            assert records(b.exact(what, x, which, own_mode=True)) == [full[int(p)] for p in which]
        assert records(b.exact(what, x, np.zeros(0, np.uint32), own_mode=True)) == []
    with pytest.raises(RuntimeError, match=rf"\b{n + 3}\b.*out of range"):
        b.exact(hip.EXACT_GLOBAL, -1, [0, n + 3], own_mode=True)
    b.close()


# ---------------------------------------------------------------- 6. sized and multi-device batches
def test_sized_and_multi_batches_in_local_start(hip):
    m, gaps, _a = kinds()["nuc"]
    pairs = seq_pairs("nuc")
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    plain = batch(hip, m, gaps, pairs, size=(32, 256), mode=hip.LOCAL_START)
    sized = hip.SizedBatchAligner(m, gaps, 0, hip.LOCAL_START, *args, percent=(0.05, 0.2))
    multi = hip.MultiBatchAligner(m, gaps, (32, 256), 0, hip.LOCAL_START, *args, devices=[0, 0])
    assert len(sized.classes()) > 1
    which = np.random.default_rng(86).integers(0, len(pairs), 70)
    Hs = seq_matrices("nuc", "local_start")
    for what, name, x in ((hip.EXACT_GLOBAL, "global", -1), (hip.EXACT_EXTEND, "extend", -1), (hip.EXACT_EXTEND, "extend", 30)):
        want = records(plain.exact(what, x, own_mode=True))
        assert want == model_records(Hs, name, x, False)
        for other in (sized, multi):
            assert records(other.exact(what, x, own_mode=True)) == want
            assert records(other.exact(what, x, which, own_mode=True)) == [want[int(p)] for p in which]
    for x in (plain, sized, multi):
        x.close()


# ---------------------------------------------------------------- 7. accuracy(own_mode=True)
def accuracy_profile_case(hip, form):
    rng = np.random.default_rng(87)
    cases = [make_profile(rng, int(rng.integers(20, 300)), int(rng.integers(20, 300)), 64, -1, form) for n in range(40)]
    pairs = synth.PairSet.from_lists([(q, b"A") for q, _p in cases])
    b = profile_batch(hip, pairs, [p for _q, p in cases], size=(32, 64))
    b.run()
    res = b.results()
    ex = b.exact(own_mode=True)
    acc = b.accuracy(own_mode=True)
    sub = b.accuracy(which=[7, 3, 3], own_mode=True)
    b.close()
    assert records(ex) == [M.own_mode(M.full_matrix_profile(q, p), "global") for q, p in cases]
    assert acc == hip.accuracy_summary(res["score"], ex, res["query_idx"], res["reference_idx"], res["status"])
    assert acc["n"] == acc["compared"] == len(cases) and acc["below"] + acc["above"] == acc["wrong"]
    assert sub["n"] == 3
    return acc


def test_accuracy_on_a_profile_batch(hip):
    """Uniform gap costs (open_C = open_R, close_C = 0, what pssm_accuracy.rs sets up): both orientations of a block's rectangles state
    the recurrence of the definition, so a run never scores above it."""
    acc = accuracy_profile_case(hip, "uniform")
    assert acc["above"] == 0


def test_accuracy_on_a_profile_batch_with_position_specific_gaps(hip):
    """With position-specific costs `above` is reported, not asserted: the definition is the recurrence of rectangles whose vectors run
    along the query (the only kind when one block covers the matrix); rectangles whose vectors run along the profile, which a 32..64
    range places too, take the runs of profile positions through the prefix scan instead (scan_block.rs:697-716), which is not the
    same recurrence once the costs depend on the position, so the reference's own result can exceed the definition's optimum. The CPU
    oracle at 32..64 does on 13 of 30 such pairs of lengths 20..300, by 1 to 9; with uniform costs on none of 30."""
    accuracy_profile_case(hip, "specific")


def test_accuracy_in_free_query_end_gaps(hip):
    """The run's score follows the reference's lane rule and may exceed the exact value: above is reported, not asserted."""
    m, gaps, _a = kinds()["nuc"]
    pairs = seq_pairs("nuc")
    b = batch(hip, m, gaps, pairs, size=(256, 256), mode=hip.FREE_QUERY_END_GAPS)
    b.run()
    acc = b.accuracy(own_mode=True)
    b.close()
    assert acc["n"] == len(pairs) and acc["compared"] + acc["skipped"] == acc["n"] and acc["below"] + acc["above"] == acc["wrong"]


# ---------------------------------------------------------------- 8. refusals
def test_refusals(hip):
    pairs = synth.make_pairs(8, 100, 5, 10, synth.AMINO, seed=540)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    m = S.static_matrix("BLOSUM62")
    profiles = [S.AAProfile.from_bytes(pairs.reference(p), 128, 2, -1, -5, 0, -5, -1) for p in range(len(pairs))]
    own = hip.EXACT_OWN_MODE
    # without the flag nothing has changed
    pb = hip.ProfileBatchAligner(profiles, (32, 64), 0, 0, pairs.pool, pairs.q_off, pairs.q_len)
    with pytest.raises(RuntimeError, match="profile batches are not supported"):
        pb.exact()
    with pytest.raises(RuntimeError, match="profile batches are not supported"):
        pb.exact(hip.EXACT_EXTEND)
    # the flag with an unknown quantity, and the paths of a profile batch
    with pytest.raises(RuntimeError, match=f"unknown quantity {7 | own}"):
        pb.exact(7 | own)
    with pytest.raises(RuntimeError, match="BA_EXACT_OWN_MODE gives scores only: no paths"):
        pb.exact_cigars(hip.EXACT_GLOBAL | own)
    assert len(pb.exact(own_mode=True)["score"]) == len(pairs)
    pb.close()
    for mode in (hip.LOCAL_START, hip.FREE_QUERY_END_GAPS, hip.FREE_QUERY_START_GAPS):
        b = hip.BatchAligner(m, (-11, -1), (128, 128), 0, mode, *args)
        with pytest.raises(RuntimeError, match="LOCAL_START"):
            b.exact()
        with pytest.raises(RuntimeError, match="BA_EXACT_OWN_MODE gives scores only: no paths"):
            b.exact_cigars(hip.EXACT_GLOBAL | own)
        b.launch()
        with pytest.raises(RuntimeError, match="in flight"):
            b.exact(own_mode=True)
        b.wait()
        assert len(b.exact(own_mode=True)["score"]) == len(pairs)
        b.close()
        # a profile batch in one of these modes: no definition yet
        pm = hip.ProfileBatchAligner(profiles, (128, 128), 0, mode, pairs.pool, pairs.q_off, pairs.q_len)
        with pytest.raises(RuntimeError, match="BA_EXACT_OWN_MODE does not cover a profile batch with BA_LOCAL_START or BA_FREE_QUERY_"):
            pm.exact(own_mode=True)
        with pytest.raises(RuntimeError, match="profile"):
            pm.exact()
        pm.close()
    # extension batches take no `what`
    ss = SeedSet([pairs.query(0), pairs.reference(0)], [0], [1], [10], [10], [8])
    eb = hip.ExtendBatchAligner(m, (-11, -1), (32, 128), 60, hip.X_DROP, *ss.args())
    with pytest.raises(RuntimeError, match="EXACT_OWN_MODE does not apply to extension batches"):
        eb.exact(own_mode=True)
    assert len(eb.exact()["score"]) == 1
    eb.close()
    # a profile pair past its guard: lengths only
    with pytest.raises(RuntimeError, match=r"pair 1 .*profile.*too long"):
        hip.exact_check_lengths_profile([100, 1 << 21], [100, 1 << 21])
