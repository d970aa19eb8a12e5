"""Optimal paths in the batch's own mode on the MI355X (ba_*_exact_paths): every record and every run of LOCAL_START / FREE_QUERY_*,
plain, profile and extension batches against the Python model of tests/exact_modes_path.py, the protocol, pair selection, sized / multi
batches, the refusals and the rescue of pairs a small block range got wrong. Every assertion covers every record."""
import functools

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests import exact_modes_path as P
from tests.test_exact_modes_path_ref import GAPS as TIE_GAPS, NUC as TIE_NUC, RESCUE_GAPS, RESCUE_NUC, RESCUE_SIZE, rescue_pairs, tie_pairs, tie_profiles
from tests.test_gpu_exact import batch, kinds
from tests.test_gpu_exact_modes import SEQ_MODES, X_DROPS, make_profile, profile_batch, seq_pairs
from tests.test_gpu_extend import SeedSet

pytestmark = pytest.mark.gpu

FIELDS = ("score", "q_start", "r_start", "q_end", "r_end", "rows")
# name -> (the model's start rule, FREE_QUERY_END_GAPS)
MODEL = {"plain": (P.GLOBAL, False), "local_start": (P.LOCAL, False), "free_query_start_gaps": (P.FREE_ROW0, False), "free_query_end_gaps": (P.GLOBAL, True),
         "local_start+free_query_end_gaps": (P.LOCAL, True), "free_query_start_gaps+free_query_end_gaps": (P.FREE_ROW0, True)}
QUANTITIES = (("global", -1),) + tuple(("extend", x) for x in X_DROPS)


def mode_bits(hip, mode):
    return 0 if mode == "plain" else SEQ_MODES[mode][0](hip)


def records(rec):
    return [tuple(int(rec[k][p]) for k in FIELDS) for p in range(len(rec["score"]))]


def split(runs, off):
    return [[int(x) for x in runs[int(off[k]):int(off[k + 1])]] for k in range(len(off) - 1)]


def what_of(hip, name):
    return hip.EXACT_GLOBAL if name == "global" else hip.EXACT_EXTEND


def sequence_case(hip, m, gaps, pairs, mode, eq):
    start, free_end = MODEL[mode]
    b = batch(hip, m, gaps, pairs, size=(256, 256), mode=mode_bits(hip, mode) | (hip.CIGAR_EQ if eq else 0))
    got = {(name, x): b.exact_paths(what_of(hip, name), x) for name, x in QUANTITIES}
    scores = {(name, x): b.exact(what_of(hip, name), x, own_mode=True) for name, x in QUANTITIES}
    b.close()
    for (name, x), (rec, runs, off) in got.items():
        want = [P.mode_paths(pairs.query(p), pairs.reference(p), m, gaps, start, free_end, name, x, eq) for p in range(len(pairs))]
        assert records(rec) == [w[0] for w in want], (name, x)
        assert split(runs, off) == [w[1] for w in want], (name, x)
        ex = scores[(name, x)]
        assert all(np.array_equal(rec[a], ex[c]) for a, c in (("score", "score"), ("q_end", "query_idx"), ("r_end", "reference_idx"), ("rows", "rows")))


# ---------------------------------------------------------------- 1. sequence modes against the model
@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("mode", ["plain", "local_start", "free_query_start_gaps", "free_query_end_gaps"])
@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_sequence_modes_equal_the_model(hip, kind, mode, eq):
    m, gaps, _a = kinds()[kind]
    sequence_case(hip, m, gaps, seq_pairs(kind), mode, eq)


@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("mode", ["local_start+free_query_end_gaps", "free_query_start_gaps+free_query_end_gaps"])
@pytest.mark.parametrize("kind", ["nuc", "aa", "bytes"])
def test_start_and_end_rules_combine(hip, kind, mode, eq):
    m, gaps, _a = kinds()[kind]
    sequence_case(hip, m, gaps, seq_pairs(kind), mode, eq)


@pytest.mark.parametrize("mode", sorted(MODEL))
def test_tie_heavy_pairs(hip, mode):
    sequence_case(hip, TIE_NUC, TIE_GAPS, synth.PairSet.from_lists(list(tie_pairs())), mode, False)


# ---------------------------------------------------------------- 2. profiles against the model
PROFILE_SHAPES = [(nq, nr) for nq in (63, 64, 65, 127, 128) for nr in (1, 64, 65, 200)] + [(1, 63), (15, 127), (200, 31), (3, 290)]


@functools.lru_cache(maxsize=None)
def profile_cases(ge):
    rng = np.random.default_rng(190 - ge)
    cases = [make_profile(rng, nq, nr, 512, ge, ("specific", "tail", "uniform")[n % 3]) for n, (nq, nr) in enumerate(PROFILE_SHAPES)]
    assert any(p.pos_aa[p.str_len, 0] == -128 for _q, p in cases)          # a never-set position
    return tuple(cases)


def profile_case(hip, cases, mode=0):
    pairs = synth.PairSet.from_lists([(q, b"A") for q, _p in cases])
    b = profile_batch(hip, pairs, [p for _q, p in cases], mode=mode)
    got = {(name, x): b.exact_paths(what_of(hip, name), x) for name, x in QUANTITIES}
    b.close()
    for (name, x), (rec, runs, off) in got.items():
        want = [P.profile_paths(q, p, name, x) for q, p in cases]
        assert records(rec) == [w[0] for w in want], (name, x)
        assert split(runs, off) == [w[1] for w in want], (name, x)
        for k, (q, p) in enumerate(cases):
            assert P.rescore_profile(split(runs, off)[k], records(rec)[k], q, p) == int(rec["score"][k])


@pytest.mark.parametrize("ge", [-1, -2])
def test_profiles_equal_the_model(hip, ge):
    profile_case(hip, profile_cases(ge))


def test_tie_heavy_profiles(hip):
    profile_case(hip, tie_profiles())


# ---------------------------------------------------------------- 3. a plain batch: exact_paths == exact_cigars
@pytest.mark.parametrize("kind", ["nuc", "bytes"])
def test_plain_batch_equals_exact_cigars(hip, kind):
    m, gaps, _a = kinds()[kind]
    pairs = seq_pairs(kind)
    b = batch(hip, m, gaps, pairs, mode=hip.CIGAR_EQ)
    for what, x in ((hip.EXACT_GLOBAL, -1), (hip.EXACT_EXTEND, -1), (hip.EXACT_EXTEND, 30)):
        rec, runs, off = b.exact_paths(what | hip.EXACT_OWN_MODE, x)
        rec0, runs0, off0 = b.exact_cigars(what, x)
        assert np.array_equal(runs, runs0) and np.array_equal(off, off0)
        assert not rec["q_start"].any() and not rec["r_start"].any()
        assert all(np.array_equal(rec[a], rec0[c]) for a, c in (("score", "score"), ("q_end", "query_idx"), ("r_end", "reference_idx"), ("rows", "rows")))
        assert records(b.exact_paths(what, x)[0]) == records(rec)               # the flag changes nothing
    b.close()


# ---------------------------------------------------------------- 4. extension batches
def extension_seeds():
    """Both strands; seeds at either end of a sequence (an empty left side, an empty right side), sides of 64 / 65 letters."""
    rng = np.random.default_rng(141)
    comp = bytes.maketrans(b"ACGT", b"TGCA")
    seqs, q_idx, r_idx, q_seed, r_seed, seed_len, strand = [], [], [], [], [], [], []
    for n, (nl, nr_) in enumerate([(0, 90), (90, 0), (0, 0), (64, 65), (65, 64), (120, 130), (30, 200), (200, 30)]):
        L = 8 + n
        r = synth.rand_str(rng, nl + L + nr_, synth.DNA)
        left = synth.mutate(rng, r[:nl], nl // 12, synth.DNA)[:nl]
        right = synth.mutate(rng, r[nl + L:], nr_ // 12, synth.DNA)
        seed = synth.mutate(rng, r[nl:nl + L], 1, synth.DNA)[:L] if n % 2 else r[nl:nl + L]
        seed = np.concatenate([seed, r[nl + len(seed):nl + L]])
        q = np.concatenate([left, seed, right]).tobytes()
        for st in (0, 1):
            seqs += [q.translate(comp)[::-1] if st else q, r.tobytes()]
            q_idx.append(len(seqs) - 2); r_idx.append(len(seqs) - 1); q_seed.append(len(left)); r_seed.append(nl); seed_len.append(L); strand.append(st)
    return SeedSet(seqs, q_idx, r_idx, q_seed, r_seed, seed_len, strand)


@pytest.mark.parametrize("eq", [False, True])
@pytest.mark.parametrize("x_drop", [-1, 30])
def test_extension_batches(hip, x_drop, eq):
    m, gaps, _a = kinds()["nuc"]
    ss = extension_seeds()
    eb = hip.ExtendBatchAligner(m, gaps, (32, 256), 60, hip.X_DROP | (hip.CIGAR_EQ if eq else 0), *ss.args(), strand=ss.strand)
    rec, runs, off = eb.exact_paths(x_drop=x_drop)
    ex = eb.exact(x_drop)
    which = np.array([5, 0, 5, 15, 2])
    rec_w, runs_w, off_w = eb.exact_paths(x_drop=x_drop, which=which)
    assert not hasattr(eb, "exact_cigars")
    eb.close()
    got = split(runs, off)
    want = [P.extend_paths(ss.q(p), ss.r(p), int(ss.q_seed[p]), int(ss.r_seed[p]), int(ss.seed_len[p]), m, gaps, x_drop, eq) for p in range(len(ss))]
    assert records(rec) == [w[0] for w in want]
    assert got == [w[1] for w in want]
    for side, at in (("left", 2), ("right", 3)):
        assert [tuple(int(rec[side][k][p]) for k in ("score", "query_idx", "reference_idx", "rows")) for p in range(len(ss))] == [w[at] for w in want]
        assert all(np.array_equal(rec[side][k], ex[side][k]) for k in ex[side])
    assert np.array_equal(rec["score"], ex["score"])
    for p in range(len(ss)):
        assert P.rescore_mode(got[p], records(rec)[p], ss.q(p), ss.r(p), m, gaps, eq) == int(rec["score"][p])
    assert records(rec_w) == [records(rec)[int(p)] for p in which] and split(runs_w, off_w) == [got[int(p)] for p in which]
    assert sum(w[2] == (0, 0, 0, 0) for w in want) >= 4 and sum(w[3] == (0, 0, 0, 0) for w in want) >= 4


# ---------------------------------------------------------------- 5. selection and protocol
def test_selection_sized_and_multi_batches(hip):
    m, gaps, _a = kinds()["nuc"]
    pairs = seq_pairs("nuc")
    n = len(pairs)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    plain = batch(hip, m, gaps, pairs, size=(32, 256), mode=hip.LOCAL_START)
    sized = hip.SizedBatchAligner(m, gaps, 0, hip.LOCAL_START, *args, percent=(0.05, 0.2))
    multi = hip.MultiBatchAligner(m, gaps, (32, 256), 0, hip.LOCAL_START, *args, devices=[0, 0])
    rng = np.random.default_rng(186)
    for what, name, x in ((hip.EXACT_GLOBAL, "global", -1), (hip.EXACT_EXTEND, "extend", 30)):
        want = [P.mode_paths(pairs.query(p), pairs.reference(p), m, gaps, P.LOCAL, False, name, x) for p in range(n)]
        for which in (None, rng.permutation(n)[:9], rng.integers(0, n, 70), np.array([n - 1, n - 1, 0, n - 1])):
            idx = range(n) if which is None else [int(p) for p in which]
            for b in (plain, sized, multi):
                rec, runs, off = b.exact_paths(what, x, which)
                assert records(rec) == [want[p][0] for p in idx] and split(runs, off) == [want[p][1] for p in idx]
        rec, runs, off = plain.exact_paths(what, x, np.zeros(0, np.uint32))
        assert records(rec) == [] and len(runs) == 0 and list(off) == [0]
    with pytest.raises(RuntimeError, match=rf"\b{n + 3}\b.*out of range"):
        plain.exact_paths(which=[0, n + 3])
    for b in (plain, sized, multi):
        b.close()


def test_two_call_protocol_and_reload(hip):
    m, gaps, _a = kinds()["nuc"]
    pairs = seq_pairs("nuc")
    n = len(pairs)
    b = batch(hip, m, gaps, pairs, mode=hip.LOCAL_START)
    L = hip.lib()
    rec, off = np.zeros(n, hip.EXACT_PATH_DTYPE), np.zeros(n + 1, np.uint64)
    assert L.ba_batch_exact_paths(b._h, hip.EXACT_GLOBAL, -1, None, 0, rec.ctypes.data, off.ctypes.data, None, 0) == 0
    total = int(off[-1])
    ms = b.exact_paths_ms()
    assert total > 0 and ms[0] > 0 and ms[1] > 0
    short = np.zeros(total - 1, np.uint32)
    assert L.ba_batch_exact_paths(b._h, hip.EXACT_GLOBAL, -1, None, 0, rec.ctypes.data, off.ctypes.data, short.ctypes.data, short.size) != 0
    assert f"holds {total - 1} runs, the request has {total}" in hip.last_error()
    runs = np.zeros(total, np.uint32)
    assert L.ba_batch_exact_paths(b._h, hip.EXACT_GLOBAL, -1, None, 0, rec.ctypes.data, off.ctypes.data, runs.ctypes.data, runs.size) == 0
    assert b.exact_paths_ms() == ms                                            # the cached copy: nothing was computed
    first = b.exact_paths(hip.EXACT_GLOBAL)
    assert np.array_equal(first[1], runs) and np.array_equal(first[2], off)
    with pytest.raises(RuntimeError, match="BA_EXACT_OWN_MODE gives scores only: no paths"):
        b.exact_cigars(hip.EXACT_GLOBAL | hip.EXACT_OWN_MODE)                  # (the older call keeps refusing this batch)
    b.reload(pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    again = b.exact_paths(hip.EXACT_GLOBAL)
    b.close()
    assert records(again[0]) == records(first[0]) and np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])


# ---------------------------------------------------------------- 6. refusals
def test_refusals(hip):
    pairs = synth.make_pairs(8, 100, 5, 10, synth.AMINO, seed=541)
    args = (pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    m = S.static_matrix("BLOSUM62")
    profiles = [S.AAProfile.from_bytes(pairs.reference(p), 128, 2, -1, -5, 0, -5, -1) for p in range(len(pairs))]
    for mode in (hip.LOCAL_START, hip.FREE_QUERY_END_GAPS, hip.FREE_QUERY_START_GAPS):
        pm = hip.ProfileBatchAligner(profiles, (128, 128), 0, mode, pairs.pool, pairs.q_off, pairs.q_len)
        with pytest.raises(RuntimeError, match="does not cover a profile batch with BA_LOCAL_START or BA_FREE_QUERY_"):
            pm.exact_paths()
        pm.close()
    b = hip.BatchAligner(m, (-11, -1), (128, 128), 0, hip.LOCAL_START, *args)
    with pytest.raises(RuntimeError, match=f"unknown quantity {7 | hip.EXACT_OWN_MODE}"):
        b.exact_paths(7)
    b.launch()
    with pytest.raises(RuntimeError, match="in flight"):
        b.exact_paths()
    b.wait()
    assert len(b.exact_paths()[0]["score"]) == len(pairs)
    b.close()
    # the cell limit: lengths only
    with pytest.raises(RuntimeError, match=r"pair 1 .*too large for a traced matrix"):
        hip.exact_trace_check_lengths([100, 1 << 16], [100, (1 << 15) + 1])
    with pytest.raises(RuntimeError, match=r"pair 0 .*profile.*too large for a traced matrix"):
        hip.exact_paths_check_lengths_profile([1 << 16], [1 << 15])


# ---------------------------------------------------------------- 7. the use case: rescue what a small block range got wrong
def test_rescue_of_wrong_local_start_pairs(hip):
    """A 200-letter insertion in the query takes the block path off the optimum when the blocks (32 .. 64) cannot span it:
    accuracy(own_mode=True) reports pairs below the optimum, and their exact paths rescore to the exact score and beat the block score.
    (tests/test_exact_modes_path_ref.py checks on the CPU that the construction yields such pairs.)"""
    m, gaps = RESCUE_NUC, RESCUE_GAPS
    pairs = synth.PairSet.from_lists(list(rescue_pairs()))
    b = batch(hip, m, gaps, pairs, size=RESCUE_SIZE, mode=hip.LOCAL_START)
    b.run()
    res = b.results()
    acc = b.accuracy(own_mode=True)
    ex = b.exact(own_mode=True)
    rec, runs, off = b.exact_paths()
    b.close()
    print("accuracy", acc)
    assert acc["below"] > 0
    got = split(runs, off)
    wrong = [p for p in range(len(pairs)) if not res["status"][p] and int(res["score"][p]) < int(ex["score"][p])]
    assert len(wrong) == acc["below"]
    for p in range(len(pairs)):
        assert P.rescore_mode(got[p], records(rec)[p], pairs.query(p), pairs.reference(p), m, gaps) == int(ex["score"][p]) == int(rec["score"][p])
    assert all(int(rec["score"][p]) > int(res["score"][p]) for p in wrong)
