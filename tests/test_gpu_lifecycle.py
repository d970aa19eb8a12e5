"""The host state machine around a launch (ba_batch_launch / ba_batch_wait, ba_sized_batch_run, ba_multibatch_run): which call is served in
which state, and that whatever is served is the oracle's. A batch has no results from its launch until a wait succeeds -- on its first launch
and on every later one, where the results of the run before are still in its buffers --, a wait that times out leaves it in flight, and a set
of batches whose run timed out serves nothing and collects what is still in flight at its next run. The refusals are host state (in_flight,
ran): they do not depend on whether the kernels have finished, so the state walk uses a tiny batch; the time-outs need a launch that outlasts
a 1 ms limit, the 20000 pairs of test_gpu_pipelines.py::test_wait_is_bounded_on_the_host, built once for this module."""
import numpy as np
import pytest

from block_aligner_amd import synth
from tests.test_gpu_parity import NUC
from tests.test_gpu_stats import check_stats, ref_stats

pytestmark = pytest.mark.gpu

GAPS = (-5, -1)
IN_FLIGHT = r"launch in flight \(ba_batch_wait first\)"
NOT_RUN = "has not been called|has not finished a run"
TIMED_OUT = "did not finish within 1 ms"
DEFAULT_LIMIT_MS = 600000
# (name, oracle mode, traced, block range, X-drop threshold)
ROUTES = (("traced", ("trace", "x_drop"), True, (32, 256), 50), ("score_only", ("x_drop",), False, (128, 512), 50))


def flags_of(hip, mode, traced):
    return sum({"trace": hip.TRACE, "x_drop": hip.X_DROP}[m] for m in mode) | (hip.CIGAR_EQ if traced else 0)


def pair_args(pairs):
    return pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len


class Want:
    """The oracle's answers for one pair set on one route, computed once: batch_align for scores, indices, run counts and runs, align per pair
    for the per-pair cell counts (the batch call returns their sum only), and the statistics and the CIGAR text those runs spell out."""

    def __init__(self, hip, oracle, pairs, mode, traced, size, x_drop, per_pair=True):
        self.pairs, self.traced, self.n = pairs, traced, len(pairs)
        ref = oracle.batch_align(NUC, *pair_args(pairs), GAPS, size, x_drop, mode, cigar_eq=traced, threads=8)
        self.ref = ref
        self.cells = self.surviving = None
        if per_pair:
            one = [oracle.align(NUC, pairs.query(p), pairs.reference(p), GAPS, size, x_drop, mode, cigar_eq=traced) for p in range(self.n)]
            self.cells = np.array([o["cells"] for o in one], np.uint64)
            self.surviving = np.array([o["surviving_cells"] for o in one], np.uint64)
            assert int(self.cells.sum()) == ref["cells"]
        if traced:
            self.runs = [ref["cig_ops"][int(ref["cig_off"][p]): int(ref["cig_off"][p]) + int(ref["cig_len"][p])] for p in range(self.n)]
            self.flat = np.concatenate(self.runs) if self.n else np.zeros(0, np.uint32)
            if per_pair:
                self.stats = [ref_stats(self.runs[p], pairs.query(p), pairs.reference(p), NUC, GAPS, int(ref["query_idx"][p]), int(ref["reference_idx"][p]))
                              for p in range(self.n)]
                self.text = [hip.runs_to_string(r) for r in self.runs]

    def check_results(self, res, what, sel=slice(None)):
        """res[sel] against the oracle: status 0, score, both indices, the run count and (where per-pair counts were computed) the cells."""
        ref = self.ref
        assert not res["status"][sel].any(), (what, np.nonzero(res["status"][sel])[0][:10])
        for got, want in (("score", ref["scores"]), ("query_idx", ref["query_idx"]), ("reference_idx", ref["reference_idx"])):
            bad = np.nonzero(res[got][sel].astype(np.int64) != want.astype(np.int64))[0]
            assert bad.size == 0, (what, got, bad[:10], res[got][sel][bad[:5]], want[bad[:5]])
        if self.traced:
            assert np.array_equal(res["cigar_len"][sel], ref["cig_len"]), what
        else:
            assert not res["cigar_len"][sel].any(), what
        if self.cells is not None:
            assert np.array_equal(res["cells"][sel], self.cells), what

    def check_runs(self, runs, off, what, sel=None):
        """The runs of the pairs `sel` (None: all, compared as one array) against the oracle's."""
        if sel is None:
            assert int(off[-1]) == self.flat.size and np.array_equal(runs[: self.flat.size], self.flat), what
            return
        for k, p in enumerate(sel):
            assert np.array_equal(runs[int(off[p]): int(off[p + 1])], self.runs[k]), (what, int(p))

    def check_all(self, b, what):
        """Every getter of a batch in a state with results: all of it is the oracle's. -> (spec_cells, skipped_cells)"""
        res = b.results()
        self.check_results(res, what)
        total = int(self.cells.sum())
        # no oracle counts these two: they are parts of the cells it does count
        spec, skipped = b.spec_cells(), b.skipped_cells()
        print(what, "spec_cells", spec, "skipped_cells", skipped, "cells", total)
        assert 0 <= spec <= total and 0 <= skipped <= total and spec + skipped <= total, (what, spec, skipped, total)
        if self.traced:
            self.check_runs(*b.cigars(res["cigar_len"]), what)
            self.check_runs(*b.cigars(), what)   # (the form that asks results() for the run counts itself)
            sv = b.surviving_cells()
            print(what, "surviving_cells", int(sv.sum()), "oracle", int(self.surviving.sum()))
            assert np.array_equal(sv, self.surviving), (what, np.nonzero(sv != self.surviving)[0][:10])
            st = b.stats()
            check_stats(st, self.stats, what)
            assert np.array_equal(st["path_score"], self.ref["scores"]), what
            assert b.text_list() == self.text, what
        else:
            assert spec == 0, (what, spec)   # (speculative rectangles are a traced X-drop batch's)
        return spec, skipped


def result_getters(b, traced):
    g = [b.results, b.spec_cells, b.skipped_cells]
    if traced:
        g += [b.cigars, lambda: b.cigars(np.ones(b.n, np.uint32)), b.surviving_cells, b.stats, b.text]
    return g


def all_refuse(b, traced, match, what):
    for k, g in enumerate(result_getters(b, traced)):
        with pytest.raises(RuntimeError, match=match):
            g()
            pytest.fail(f"{what}: getter {k} was served")


def in_flight_refusals(b, traced, pairs, what):
    all_refuse(b, traced, IN_FLIGHT, what)
    with pytest.raises(RuntimeError, match=IN_FLIGHT):
        b.launch()
    with pytest.raises(RuntimeError, match=IN_FLIGHT):
        b.run()
    with pytest.raises(RuntimeError, match=IN_FLIGHT):
        b.reload(*pair_args(pairs))
    # host state answers in every state
    assert b.info()["kernel"] in b.KERNELS and b.info()["grid"] > 0 and b.retried() >= 0


@pytest.fixture(scope="module")
def small_pairs():
    return synth.make_pairs(64, (100, 900), (0, 60), 10, synth.DNA, seed=9)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_getter_in_every_state(hip, oracle, small_pairs, route):
    """One batch walked through created, launched, waited, launched again, waited, a refused reload, a reload and a run: in every state
    every getter either refuses with the state's message or returns the oracle's values. The fourth state is the one a stale `ran` got
    wrong: on a second launch the getters served the buffers the kernels were writing."""
    name, mode, traced, size, x_drop = route
    pairs = small_pairs
    want = Want(hip, oracle, pairs, mode, traced, size, x_drop)
    b = hip.BatchAligner(NUC, GAPS, size, x_drop, flags_of(hip, mode, traced), *pair_args(pairs))
    try:
        # created
        all_refuse(b, traced, NOT_RUN, (name, "created"))
        with pytest.raises(RuntimeError, match="nothing was launched"):
            b.wait()
        with pytest.raises(RuntimeError, match="between ba_batch_launch and ba_batch_wait" if traced else "without BA_TRACE"):
            b.compact_cigars()
        assert b.retried() == 0
        # launched, first launch
        b.launch()
        in_flight_refusals(b, traced, pairs, (name, "first launch"))
        if traced:
            b.compact_cigars()   # (this run's cigars() is then a copy of the gathered runs; the second run's gathers on demand)
        in_flight_refusals(b, traced, pairs, (name, "first launch, gather queued"))
        # waited
        assert b.wait() > 0
        first = want.check_all(b, (name, "first wait"))
        with pytest.raises(RuntimeError, match="nothing was launched"):
            b.wait()
        # launched again: the buffers still hold the first run's results, and none of them is served
        b.launch()
        in_flight_refusals(b, traced, pairs, (name, "second launch"))
        # waited
        assert b.wait() > 0
        assert want.check_all(b, (name, "second wait")) == first
        assert isinstance(b.retried(), int) and b.retried() >= 0
        # a reload that is refused before it changes anything (more pairs than the batch was created for): the batch is as it was
        twice = [np.concatenate([a, a]) for a in pair_args(pairs)[1:]]
        with pytest.raises(RuntimeError, match="exceed the batch's capacity"):
            b.reload(pairs.pool, *twice)
        assert b.n == len(pairs)
        assert want.check_all(b, (name, "after the refused reload")) == first
        # reloaded with a smaller set: no results until it has run
        sub = pairs.subset(np.arange(7, 47))
        want_sub = Want(hip, oracle, sub, mode, traced, size, x_drop)
        b.reload(*pair_args(sub))
        all_refuse(b, traced, NOT_RUN, (name, "reloaded"))
        with pytest.raises(RuntimeError, match="nothing was launched"):
            b.wait()
        assert b.run() > 0
        want_sub.check_all(b, (name, "reloaded and run"))
    finally:
        b.close()


def test_compact_cigars_on_every_run(hip, oracle, small_pairs):
    """launch, compact_cigars, wait, cigars -- the gather queued behind the kernels -- on the first run and on the second: both times the
    runs are the oracle's, from the device buffer and from page-locked host memory; in between, while in flight, cigars() is refused before
    it reads the gather's total."""
    name, mode, traced, size, x_drop = ROUTES[0]
    pairs = small_pairs
    want = Want(hip, oracle, pairs, mode, traced, size, x_drop, per_pair=False)
    b = hip.BatchAligner(NUC, GAPS, size, x_drop, flags_of(hip, mode, traced), *pair_args(pairs))
    pinned = hip.pinned_array(int(want.flat.size) + 64)
    try:
        for rnd, out in enumerate((None, None, pinned, pinned)):
            b.launch()
            b.compact_cigars(out)
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.cigars(want.ref["cig_len"], out=out)
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.results()
            b.wait()
            res = b.results()
            want.check_results(res, ("compact", rnd))
            want.check_runs(*b.cigars(res["cigar_len"], out=out), ("compact", rnd))
            if out is not None:
                assert np.array_equal(pinned[: want.flat.size], want.flat), rnd   # (the gather wrote the caller's buffer itself)
                pinned[:] = 0
    finally:
        b.close()
        hip.free_pinned(pinned)


# ---------------------------------------------------------------- launches that outlast a 1 ms limit

BIG_N, BIG_STEP = 20000, 200
BIG_SIZES = ((128, 512), (128, 1024))
BIG_MODE = ("trace", "x_drop")


class Big:
    """The pairs of test_wait_is_bounded_on_the_host and the oracle's answers for every 200th of them, per block range, computed on demand
    and once."""

    def __init__(self, hip, oracle):
        self.hip, self.oracle = hip, oracle
        self.pairs = synth.make_pairs(BIG_N, 3000, 300, 100, synth.DNA, seed=99, workers=1)
        self._want = {}

    def want(self, first, size):
        """Pairs first, first + 200, ... at the block range `size`."""
        if (first, size) not in self._want:
            idx = np.arange(first, BIG_N, BIG_STEP)
            self._want[first, size] = (idx, Want(self.hip, self.oracle, self.pairs.subset(idx), BIG_MODE, True, size, 100, per_pair=False))
        return self._want[first, size]


@pytest.fixture(scope="module")
def big(hip, oracle):
    return Big(hip, oracle)


def same_results(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a) and a.keys() == b.keys()


def test_timed_out_wait_on_a_later_launch(hip, oracle, big):
    """A batch that has run once is launched again under a 1 ms limit: the wait times out, the batch stays in flight, and until a later
    wait succeeds it serves nothing -- not the first run's results either, which its buffers still held when the launch began. Then the
    second run's results are the first's, and the oracle's."""
    pairs = big.pairs
    b = hip.BatchAligner(NUC, GAPS, BIG_SIZES[0], 100, flags_of(hip, BIG_MODE, True), *pair_args(pairs))
    try:
        b.run()
        res1 = b.results()
        runs1, off1 = b.cigars(res1["cigar_len"])
        try:
            hip.lib().ba_set_wait_limit_ms(1)
            b.launch()
            with pytest.raises(RuntimeError, match=TIMED_OUT):
                b.wait()
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.results()
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.cigars(res1["cigar_len"])
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.launch()
            with pytest.raises(RuntimeError, match=IN_FLIGHT):
                b.reload(*pair_args(pairs))
        finally:
            hip.lib().ba_set_wait_limit_ms(DEFAULT_LIMIT_MS)
        assert b.wait() > 1.0
        res2 = b.results()
        assert same_results(res1, res2)
        runs2, off2 = b.cigars(res2["cigar_len"])
        assert np.array_equal(off1, off2) and np.array_equal(runs1, runs2)
        idx, want = big.want(0, BIG_SIZES[0])
        want.check_results(res2, "second run", idx)
        want.check_runs(runs2, off2, "second run", idx)
    finally:
        hip.lib().ba_set_wait_limit_ms(DEFAULT_LIMIT_MS)
        try:
            b.wait()   # (a failure above may have left the launch in flight: no batch is closed that was not waited for)
        except RuntimeError:
            pass
        b.close()


SET_REFUSED = "in flight|last run did not complete"


def set_after_a_timed_out_run(hip, s, checks):
    """run; run under a 1 ms limit (times out); every getter of the set refuses; the very next run under the default limit collects what
    was left in flight and runs afresh: its results are the first run's and, for the pairs of `checks` [(indices, Want)], the oracle's."""
    s.run()
    res1 = s.results()
    runs1, off1 = s.cigars(res1["cigar_len"])
    assert not res1["status"].any()
    try:
        hip.lib().ba_set_wait_limit_ms(1)
        with pytest.raises(RuntimeError, match=TIMED_OUT):
            s.run()
        for g in (s.results, lambda: s.cigars(res1["cigar_len"]), s.cigars, s.stats, s.text, s.exact):
            with pytest.raises(RuntimeError, match=SET_REFUSED):
                g()
        with pytest.raises(RuntimeError, match=TIMED_OUT):   # still running: the next run says so again and launches nothing
            s.run()
        with pytest.raises(RuntimeError, match=SET_REFUSED):
            s.results()
    finally:
        hip.lib().ba_set_wait_limit_ms(DEFAULT_LIMIT_MS)
    assert s.run() > 1.0
    res2 = s.results()
    assert same_results(res1, res2)
    runs2, off2 = s.cigars(res2["cigar_len"])
    assert np.array_equal(off1, off2) and np.array_equal(runs1, runs2)
    for idx, want in checks:
        want.check_results(res2, "run after the timed-out one", idx)
        want.check_runs(runs2, off2, "run after the timed-out one", idx)
    return res2


def close_set(hip, s):
    hip.lib().ba_set_wait_limit_ms(DEFAULT_LIMIT_MS)
    try:
        s.run()   # (collects whatever a failure above left in flight)
    except RuntimeError:
        pass
    s.close()


def test_sized_set_runs_again_after_a_timed_out_run(hip, oracle, big):
    """Two block ranges. Where their launches' waves wait for each other the second is launched after the first: a time-out in the first
    then leaves it in flight and the second never launched, with the results of the run before still marked as run. The set serves none of
    it, and the next run does not fail on "already has a launch in flight"."""
    pairs = big.pairs
    sizes = np.array([BIG_SIZES[p % 2] for p in range(BIG_N)], np.uint64)
    s = hip.SizedBatchAligner(NUC, GAPS, 100, flags_of(hip, BIG_MODE, True), *pair_args(pairs), sizes=sizes)
    try:
        assert len(s.classes()) == 2
        # every 200th pair lies in the first range: the pairs after them, all in the second, are compared too
        set_after_a_timed_out_run(hip, s, [big.want(0, BIG_SIZES[0]), big.want(1, BIG_SIZES[1])])
        assert sorted(c[:3] for c in s.classes()) == [(128, 512, BIG_N // 2), (128, 1024, BIG_N // 2)]
    finally:
        close_set(hip, s)


def test_multibatch_runs_again_after_a_timed_out_run(hip, oracle, big):
    """Two slices on one device, launched together: after a run that timed out the set serves nothing, kernel_ms() included, and the next
    run collects both launches before it starts its own."""
    s = hip.MultiBatchAligner(NUC, GAPS, BIG_SIZES[0], 100, flags_of(hip, BIG_MODE, True), *pair_args(big.pairs), devices=[0, 0])
    try:
        set_after_a_timed_out_run(hip, s, [big.want(0, BIG_SIZES[0])])
        assert len(s.kernel_ms()) == 2 and (s.kernel_ms() > 0).all()
    finally:
        close_set(hip, s)
