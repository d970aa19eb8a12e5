"""The whole-wave walk's diagonal pass crosses the staged rectangles (round 11, ba_driver.hpp walk_wave).

In state D lane k looks at cell (i - k, j - k) in whichever staged record holds it -- the first one from the current record on, found by a running
maximum over the records' lanes and an owner table in LDS -- so a run of matches no longer stops at the edge of an 8-cell-wide rectangle. What can
go wrong there is the owner of a cell next to an edge, the layout and direction of the owner's trace words, a run that ends where the staged
records end, a rectangle that does not fit the LDS region and is walked out of global memory, and the matrix edge.

block_cigar_* of the handle API is walk_wave on per-pair rectangles: the shapes of test_gpu_boundary.py::test_whole_wave_walk_takes_diagonal_runs
at four size ranges, plus identical sequences around 64 bases, a single-base gap at 0, 1, 7 and 8 cells beyond a rectangle's edge (right and down
strips), a mismatch in a rectangle's first and last cell, a 600..900-base indel (a grown rectangle larger than the LDS region in the middle of a
run), a path that meets i = 0 or j = 0 inside a run, and walks from interior cells of the path, which give a prefix of the whole CIGAR. k_multi's
slot rectangles (the other layout, the order of its registers) are walked by the helper waves and by the solo driver: one batch of 600 pairs of
config 3's shape at a tenth of its length on few workgroups, every pair against the oracle, with and without the hand-off ring and in the
large-pool form. Every CIGAR is compared with the oracle's, with and without = / X."""
import re

import numpy as np
import pytest

from block_aligner_amd import scores as S, synth
from tests.test_gpu_parity import NUC

pytestmark = pytest.mark.gpu

GAPS = (-5, -1)
SIZES = [(32, 32), (128, 128), (32, 1024), (128, 1024)]


def other_base(x):
    return synth.DNA[(np.searchsorted(synth.DNA, x) + 1) % 4]


def cut(x, at):
    return np.concatenate([x[:at], x[at + 1:]])


def gap_coverage(seen, cigar, qi, ri, blocks):
    """seen: (orientation, K) of every gap cell of the path -- the strip that holds the cell by the walk's rule (the first record from the top whose
    corner lies at or above-left of it) and K = min(i - row, j - col), the diagonal cells left before that strip's edge."""
    i, j = qi, ri
    for ln, op in reversed(re.findall(r"(\d+)([MIDX=])", cigar)):
        for _ in range(int(ln)):
            if op in "ID":
                for row, col, w, h in reversed(blocks):
                    if i >= row and j >= col:
                        if w and h and w != h:
                            seen.add(("right" if w < h else "down", min(i - row, j - col)))
                        break
            i -= op in "M=XI"
            j -= op in "M=XD"


def handle_cases(size):
    rng = np.random.default_rng(7000 + size[0] + size[1])
    base = synth.rand_str(rng, 1500, synth.DNA)
    cases = []
    for n in (63, 64, 65, 129, 1500):                       # runs longer than the wave; runs that end where 64 staged records end
        cases.append((base[:n], base[:n].copy()))
    for k in (2, 3, 5, 17):                                  # = / X runs of every length
        other = base.copy(); other[::k] = other_base(other[::k])
        cases.append((base, other))
    B = size[0]
    # a single-base gap 0, 1, 7, 8 cells beyond a rectangle's edge (strips are 8 cells across and their edges lie at multiples of 8 along the main
    # diagonal), in either sequence. A path on the main diagonal lies in down strips; an earlier single-base gap in the query or in the
    # reference moves it off the diagonal, into right strips or a cell deeper into the down strips. gap_coverage() checks what was reached.
    for edge in (B, 2 * B, 5 * B):
        for d in (0, 1, 7, 8):
            at = edge + d
            for pre in (None, "q", "r"):
                for side in ("q", "r"):
                    q, r = base[:1200], base[:1200]
                    q, r = (cut(q, at), r) if side == "q" else (q, cut(r, at))
                    if pre == "q":
                        q = cut(q, 40)
                    if pre == "r":
                        r = cut(r, 40)
                    cases.append((q, r))
    for at in (B - 1, B, 2 * B - 1, 2 * B, 8 * B - 1, 8 * B):   # a mismatch in the last / first cell of a rectangle
        other = base[:1200].copy(); other[at] = other_base(other[at])
        cases.append((base[:1200], other))
    for gap in (600, 900):                                   # a grown rectangle larger than the LDS region, in the middle of a run
        cases.append((base, np.concatenate([base[:500], synth.rand_str(rng, gap, synth.DNA), base[500:]])))
        cases.append((np.concatenate([base[:500], synth.rand_str(rng, gap, synth.DNA), base[500:]]), base))
    cases.append((base[:700], np.concatenate([base[:700], synth.rand_str(rng, 300, synth.DNA)])))   # the path ends on the matrix edge
    cases.append((base[40:700], base[:700]))                 # the path reaches i = 0 inside a run (leading reference bases are a gap)
    cases.append((base[:700], base[40:700]))                 # ... and j = 0
    return cases


def expand(cigar):
    return "".join(op * int(n) for n, op in re.findall(r"(\d+)([MIDX=])", cigar))


def compress(ops):
    return "".join(f"{len(m.group(0))}{m.group(1)}" for m in re.finditer(r"(.)\1*", ops))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_handle_walks(hip, oracle, size):
    m = S.NucMatrix.new_simple(2, -3)
    crossed, seen = 0, set()
    for q, r in handle_cases(size):
        qb, rb = q.astype(np.uint8).tobytes(), r.astype(np.uint8).tobytes()
        pq = hip.PaddedBytes.from_bytes(qb, size[1], S.NucMatrix); pr = hip.PaddedBytes.from_bytes(rb, size[1], S.NucMatrix)
        a = hip.Block(len(qb), len(rb), size[1], trace=True)
        a.align(pq, pr, m, S.Gaps(*GAPS), size, 0)
        res = a.res()
        full = {}
        for eq in (True, False):
            ref = oracle.align(m, qb, rb, GAPS, size, 0, ("trace",), cigar_eq=eq)
            assert (res.score, res.query_idx, res.reference_idx) == (ref["score"], ref["query_idx"], ref["reference_idx"])
            cg = hip.Cigar(res.query_idx, res.reference_idx)
            if eq:
                a.trace().cigar_eq(pq, pr, res.query_idx, res.reference_idx, cg)
            else:
                a.trace().cigar(res.query_idx, res.reference_idx, cg)
            assert str(cg) == ref["cigar"], (size, len(qb), len(rb), eq, str(cg)[:120], ref["cigar"][:120])
            full[eq] = expand(ref["cigar"])
        gap_coverage(seen, ref["cigar"], ref["query_idx"], ref["reference_idx"], oracle.align_blocks(m, qb, rb, GAPS, size, 0, ("trace",)))
        crossed += max(int(n) for n in re.findall(r"(\d+)M", compress(full[False]))) > size[0]
        # walks from interior cells of the path: a cell that the path leaves forwards by a diagonal move is reached in state D, and the walk from
        # there gives the whole CIGAR's prefix
        ops = full[False]
        ci = np.cumsum([c in "MI" for c in ops]); cj = np.cumsum([c in "MD" for c in ops])
        picks = [t for t in (1, 63, 64, 65, 511, 600, len(ops) - 1) if 0 < t < len(ops) and ops[t] == "M"]
        for t in picks:
            i, j = int(ci[t - 1]), int(cj[t - 1])
            for eq in (True, False):
                part = hip.Cigar(i, j)
                if eq:
                    a.trace().cigar_eq(pq, pr, i, j, part)
                else:
                    a.trace().cigar(i, j, part)
                assert str(part) == compress(full[eq][:t]), (size, len(qb), len(rb), t, eq)
    assert crossed > 10   # (runs longer than the smallest rectangle is wide: they were taken across rectangles)
    # gaps met 0, 1 and 7 cells before the edge of a right strip and of a down strip (8 cells: 0 of the next strip)
    for strip in ("right", "down"):
        assert {0, 1, 7} <= {k for o, k in seen if o == strip}, (strip, sorted(seen))


# ---- k_multi's slot rectangles: the helper waves' walks and the solo driver's
_batch = {}


def c3_tenth():
    if "pairs" not in _batch:
        _batch["pairs"] = synth.make_pairs(600, 1000, 100, 50, synth.DNA, seed=1111)   # config 3 at a tenth of its length: an edit every ten bases, 2/3 of them indels
    return _batch["pairs"]


def c3_reference(oracle, eq):
    if eq not in _batch:
        p = c3_tenth()
        _batch[eq] = oracle.batch_align(NUC, p.pool, p.q_off, p.q_len, p.r_off, p.r_len, GAPS, (128, 1024), 100, ("trace", "x_drop"), cigar_eq=eq, threads=16)
    return _batch[eq]


def run_and_check(H, oracle, eq):
    p = c3_tenth()
    b = H.BatchAligner(NUC, GAPS, (128, 1024), 100, H.TRACE | H.X_DROP | (H.CIGAR_EQ if eq else 0), p.pool, p.q_off, p.q_len, p.r_off, p.r_len)
    assert b.info()["kernel"] == "k_multi", b.info()
    b.run()
    res = b.results()
    runs, off = b.cigars(res["cigar_len"])
    ref = c3_reference(oracle, eq)
    assert not res["status"].any(), np.nonzero(res["status"])[0][:10]
    for got, want in (("score", "scores"), ("query_idx", "query_idx"), ("reference_idx", "reference_idx"), ("cigar_len", "cig_len")):
        bad = np.nonzero(res[got].astype(np.int64) != np.asarray(ref[want]).astype(np.int64))[0]
        assert bad.size == 0, (got, bad[:10])
    for k in range(len(p)):
        want = ref["cig_ops"][int(ref["cig_off"][k]): int(ref["cig_off"][k]) + int(ref["cig_len"][k])]
        assert np.array_equal(runs[int(off[k]): int(off[k + 1])], want), (k, eq)
    b.close()


@pytest.fixture
def few_workgroups(devlib, monkeypatch):
    monkeypatch.setenv("BA_FORCE_MULTI", "1")
    monkeypatch.setenv("BA_MQ_GEOM", "0")
    monkeypatch.setenv("BA_GRID", "4")
    monkeypatch.setenv("BA_WORK_CHUNK", "4")
    return devlib


@pytest.mark.parametrize("pool64", [False, True])
@pytest.mark.parametrize("ring", [True, False])
def test_slot_rectangles(few_workgroups, monkeypatch, oracle, ring, pool64):
    """ring: traceback waves and, at the batch's end, the emptied fill waves' whole-wave walks (traceback_helper_wave); without it every pair is
    walked by the wave that filled it (the solo driver's walk_wave)."""
    if ring:
        monkeypatch.setenv("BA_FORCE_TB", "1")
        monkeypatch.setenv("BA_WGS_PER_CU", "1")
        # the dedicated traceback waves stop taking tickets at the batch's last BA_TB_RESERVE hand-offs (traceback_consumer: reserve_from): those are
        # walked by emptied fill waves, whole-wave. (The library has no counter of helper walks outside its timing build; 24 is below the host's cap
        # for the 28 or more fill waves of four workgroups.)
        monkeypatch.setenv("BA_TB_RESERVE", "24")
    if pool64:
        monkeypatch.setenv("BA_POOL64", "1")
    for eq in (True, False):
        run_and_check(few_workgroups, oracle, eq)
