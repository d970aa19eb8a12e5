"""The end clip on the device (ba_driver.hpp run()): under X-drop the block that covers both sequence ends is the pair's
last, and its rectangles stop at the end of their column sequence -- the untraced rectangles of a speculative chain in the traced kernels,
every rectangle in the score-only kernels. Nothing of it may show: every pair of every batch is compared with the oracle on score, both end
positions, `cells` (the reference's count: the skipped cells are added back) and, where traced, every CIGAR run; `skipped_cells()` says
whether the clip ran at all.

Per-pair `cells`: the oracle's batch call returns their sum only, so the batches of a few hundred pairs ask the oracle pair by pair as well and
the 13 000-pair batches do that for a sample."""
import numpy as np
import pytest

from block_aligner_amd import scores as S
from block_aligner_amd import synth
from tests.end_clip_pairs import clip_pairs
from tests.test_gpu_parity import NUC
from tests.test_gpu_pipelines import MODES, assert_batch_equals, mode_bits

pytestmark = pytest.mark.gpu

X_DROP = 250   # (tests/test_end_clip_model.py: at 100 a third of such pairs reach a covering block, at 250 nearly all)


def run_checked(H, oracle, pairs, matrix, gaps, size, x_drop, mode, what, cells_every=1, batch=None):
    """One batch against the oracle; returns (results, CIGAR runs or None, skipped_cells())."""
    b = batch or H.BatchAligner(matrix, gaps, size, x_drop, mode_bits(H, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    b.run()
    res = b.results()
    ref = oracle.batch_align(matrix, pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len, gaps, size, x_drop, mode,
                             cigar_eq="trace" in mode, threads=16)
    assert_batch_equals(H, b, res, ref, pairs, matrix if matrix.KIND != 2 else None, gaps, mode, what)
    plain = tuple(m for m in mode if m != "trace")
    for p in range(0, len(pairs), cells_every):
        one = oracle.align(matrix, pairs.query(p), pairs.reference(p), gaps, size, x_drop, plain)
        assert int(res["cells"][p]) == one["cells"], (what, p, int(res["cells"][p]), one["cells"])
    runs = b.cigars(res["cigar_len"])[0] if "trace" in mode else None
    skipped = b.skipped_cells()
    assert skipped <= int(res["cells"].sum()), what
    b.close()
    return res, runs, skipped


@pytest.fixture(scope="module")
def ragged():
    """600 pairs of 150..700 bases, independent tails of 0..600, every fifth with a long indel near its end."""
    return synth.PairSet.from_lists(clip_pairs(600, synth.DNA, 31, length=(150, 700)))


@pytest.mark.parametrize("size", [(128, 512), (128, 1024), (32, 256)])
@pytest.mark.parametrize("mode", MODES)
def test_per_pair_kernel(hip, oracle, ragged, mode, size):
    res, _, skipped = run_checked(hip, oracle, ragged, NUC, (-5, -1), size, X_DROP if "x_drop" in mode else 0, mode, ("ragged", mode, size))
    if "x_drop" in mode:
        assert skipped > 0, (mode, size)
    else:
        assert skipped == 0, (mode, size, skipped)


@pytest.mark.parametrize("mode", [("trace", "x_drop"), ("x_drop",)])
def test_k_multi_solo_mode(hip, oracle, mode):
    """13 000 pairs of 1500..3000 bases with 300-base tails at (128, 1024): four pairs to a wave in slots, the closing grows in solo mode."""
    pairs = synth.make_pairs(13000, (1500, 3000), (60, 300), 300, synth.DNA, seed=4242, indels=1, indel_len=(10, 120))
    b = hip.BatchAligner(NUC, (-5, -1), (128, 1024), 100, mode_bits(hip, mode, True), pairs.pool, pairs.q_off, pairs.q_len, pairs.r_off, pairs.r_len)
    assert b.info()["kernel"] == "k_multi"
    _, _, skipped = run_checked(hip, oracle, pairs, NUC, (-5, -1), (128, 1024), 100, mode, ("k_multi", mode), cells_every=53, batch=b)
    assert skipped > 0


def last_block_of(q, r, gaps, size, x_drop):
    """(si, sj, block size) of the block the reference's driver ends in, from the Python mirror (tests/driver_model.py)."""
    from tests.driver_model import Model

    class Geometry(Model):
        def _place(self, seqv, lenv, seqc, lenc, start_i, start_j, width, height, *rest):
            right = rest[-1]
            if rest[2] is not self.temp1 and right:   # the right part of a grow: the block is (start_i, start_j - (height - width)), height cells
                self.last_grow = (start_i, start_j - (height - width), height)
            return super()._place(seqv, lenv, seqc, lenc, start_i, start_j, width, height, *rest)

    m = Geometry(x_drop=True)
    m.align(q, r, NUC, gaps, size, x_drop)
    return m.last_grow, m.end_block_size


def test_edge_widths_by_construction(hip, oracle):
    """Construction: q = r = 400 random bases (an exact match), then 1000 unrelated random bases on each. With X-drop 250 at (128, 1024) the best
    score is the end of the match and the alignment closes with the grows 128 -> 1024 from the checkpoint (si, sj) taken there; the Python
    mirror of the driver tells (si, sj) for the untruncated pair. The grow to 1024 has a down part of rw = 512 columns = query rows si + 512 ..
    and a right part of rw = 512 columns = reference columns sj + 512 ..; row qlen and column rlen hold the last residues, so cutting the tails
    to qlen = si + 512 + d and rlen = sj + 512 + e leaves exactly d + 1 and e + 1 live columns in the two parts: d, e in {0, 510, 511} give
    clipped widths of 1, rw - 1 and rw, d = 0 is also the case qlen - si <= 512 in a 1024-cell block (a down part with a single live column),
    and at 512 the block no longer covers that end and nothing is clipped. A width of 0 cannot come out of a grow's down part (with
    qlen < si + 512 the 512-cell block does not grow: it shifts right to its end, d = -1; aligned and compared all the same); the swapped pairs
    put every cut on the other part. The mirror is asked again for every cut pair whether it still ends in that 1024-cell block at (si, sj)."""
    rng = np.random.default_rng(99)
    core = synth.rand_str(rng, 400, synth.DNA)
    tq, tr = synth.rand_str(rng, 1000, synth.DNA), synth.rand_str(rng, 1000, synth.DNA)
    gaps, size = (-5, -1), (128, 1024)
    full_q, full_r = np.concatenate([core, tq]), np.concatenate([core, tr])
    (si, sj, bs), end_bs = last_block_of(full_q.tobytes(), full_r.tobytes(), gaps, size, X_DROP)
    assert bs == 1024 and end_bs == 1024, (si, sj, bs, end_bs)
    lists, cuts = [], []
    for d in (-1, 0, 1, 510, 511, 512):
        for e in (0, 1, 510, 511, 512):
            qlen, rlen = si + 512 + d, sj + 512 + e
            if qlen < 400 or rlen < 400 or qlen > len(full_q) or rlen > len(full_r):
                continue
            q, r = full_q[:qlen].tobytes(), full_r[:rlen].tobytes()
            geo, _ = last_block_of(q, r, gaps, size, X_DROP)
            if geo == (si, sj, 1024):   # (a cut that moves the last block -- d = e = 512 ends elsewhere -- is still aligned and compared below)
                cuts.append((d, e))
            lists.append((q, r)); lists.append((r, q))
    assert {(0, 0), (1, 1), (510, 510), (511, 511), (0, 511), (511, 0), (510, 1)} <= set(cuts), cuts
    pairs = synth.PairSet.from_lists(lists)
    for mode in (("x_drop",), ("trace", "x_drop")):
        _, _, skipped = run_checked(hip, oracle, pairs, NUC, gaps, size, X_DROP, mode, ("edge widths", mode))
        assert skipped > 0


def test_the_clipped_block_finds_a_new_best(hip, oracle):
    """400 pairs: a common prefix of 300..600 bases, 250..400 random bases inserted in one of the two, a common suffix of 120..200 bases. The
    match resumes inside the last grow (128 -> 1024 from the end of the prefix): where the suffix outweighs the gap the clipped, untraced block
    raises the best, the chain is rolled back and repeated traced and unclipped. Some pairs must end in the suffix.
    (What the Python mirror of the driver shows for these pairs: the shorter sequence ends 120..200 bases behind the prefix, so the block stops
    growing at 256 or 512 cells -- `sj + block_size > rlen` forces shift steps -- and the block that covers both ends is reached by a shift
    step of 8 columns, 2..7 of them live. The score-only kernels clip that step; the traced kernels clip untraced grows only, so for them
    this batch checks that nothing changed and `skipped_cells()` may be 0. Roll-backs out of a clipped grow are in the ragged batches above.)"""
    rng = np.random.default_rng(1717)
    lists, pre = [], []
    for p in range(400):
        a = synth.rand_str(rng, int(rng.integers(300, 601)), synth.DNA)
        ins = synth.rand_str(rng, int(rng.integers(250, 401)), synth.DNA)
        z = synth.rand_str(rng, int(rng.integers(120, 201)), synth.DNA)
        q, r = np.concatenate([a, ins, z]), np.concatenate([a, z])
        if p & 1:
            q, r = r, q
        lists.append((q.astype(np.uint8).tobytes(), r.astype(np.uint8).tobytes())); pre.append(len(a))
    pairs = synth.PairSet.from_lists(lists)
    pre = np.asarray(pre)
    for mode in (("trace", "x_drop"), ("x_drop",)):
        res, _, skipped = run_checked(hip, oracle, pairs, NUC, (-5, -1), (128, 1024), 450, mode, ("new best in the last block", mode))
        in_suffix = int(((res["query_idx"] > pre + 100) & (res["reference_idx"] > pre + 100)).sum())
        assert in_suffix > 0, in_suffix
        if "trace" not in mode:   # (see the docstring: here the last block is reached by a shift step, which only the score-only kernels clip)
            assert skipped > 0


def test_clipping_is_off_for_other_matrices(hip, oracle, ragged):
    """NucMatrices whose padding row holds a non-negative entry, and a byte matrix (padding equals padding: a match).
    'Z' against 'B' = 0 is an entry no DNA sequence reads (row 'Z' & 7, column 'B' & 15): results are the stock matrix's, traced or not, but the
    host's scan is over the whole row and column and leaves the clip off. 'Z' against 'A' = 0 is read: a best score may now sit in the padding,
    where the reference's traceback refuses to start ("end position must be in bounds"), so that matrix runs score-only."""
    cases = []
    m = S.NucMatrix.new_simple(2, -3)
    m.set(ord("Z"), ord("B"), 0)
    cases += [(m, ("x_drop",)), (m, ("trace", "x_drop"))]
    m = S.NucMatrix.new_simple(2, -3)
    m.set(ord("Z"), ord("A"), 0)
    cases += [(m, ("x_drop",))]
    for k, (m, mode) in enumerate(cases):
        _, _, skipped = run_checked(hip, oracle, ragged, m, (-5, -1), (128, 1024), X_DROP, mode, ("padding scores 0", k, mode))
        assert skipped == 0, skipped
    byt = synth.PairSet.from_lists(clip_pairs(200, np.frombuffer(b"abcdefghij", np.uint8), 33, length=(150, 700)))
    _, _, skipped = run_checked(hip, oracle, byt, S.BYTES1, (-2, -1), (128, 1024), 60, ("x_drop",), ("byte matrix", "x_drop"), cells_every=7)
    assert skipped == 0, skipped


@pytest.mark.parametrize("mode", [("trace", "x_drop"), ("x_drop",)])
def test_development_switch_ab(hip, oracle, devlib, monkeypatch, ragged, mode):
    """The development library with and without BA_NO_END_CLIP: the same result arrays and CIGAR runs, and nothing skipped with the switch."""
    res, runs, skipped = run_checked(hip, oracle, ragged, NUC, (-5, -1), (128, 1024), X_DROP, mode, ("clip on", mode), cells_every=600)
    monkeypatch.setenv("BA_NO_END_CLIP", "1")
    res2, runs2, skipped2 = run_checked(hip, oracle, ragged, NUC, (-5, -1), (128, 1024), X_DROP, mode, ("clip off", mode), cells_every=600)
    assert skipped > 0 and skipped2 == 0, (skipped, skipped2)
    for k in ("score", "query_idx", "reference_idx", "cells", "cigar_len", "status"):
        assert np.array_equal(res[k], res2[k]), k
    if runs is not None:
        assert np.array_equal(runs, runs2)
