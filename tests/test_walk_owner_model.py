"""The owner rule of the whole-wave walk's diagonal pass (ba_driver.hpp walk_wave, round 11), as a model checked against the plain search.

In state D lane k of the walking wave looks at cell (i - k, j - k). The cell's rectangle is the walk's own choice: the first record from the
top of the stack, not above the current one, whose corner (bi, bj) lies at or above-left of the cell. The kernel does not search per lane: lane a
holds staged record a, computes K_a = min(i - bi_a, j - bj_a) (signed; -1 for a record above the current one or one that is not staged), takes a
running maximum from the current record on, and record a owns the k that it is the first to reach: prev_a < k <= pm_a. A lane beyond the last
maximum has no staged owner. A record that was never traced keeps its K: the lane that it owns ends the run, so that the code behind the pass
meets that cell itself and reports the lost traceback (hiding the record from the maximum would hand its cells to a record below it).

Record stacks come from the oracle's Trace::blocks() for seeded DNA pairs with substitutions, single-base and long indels (the long ones make the
block grow; X-drop batches end with the end game's records), at both ends of the size ranges in use. Diagonals start at path cells and at random
interior cells; the staged window and the current record are drawn at random among the legal ones."""
import re

import numpy as np

from block_aligner_amd import scores as S, synth

GAPS, X_DROP = (-5, -1), 100
SIZES = [(32, 256), (128, 1024)]
N_PAIRS = 200


def owners_model(corners, cur, i, j):
    """corners: the staged records from the top of the stack, (bi, bj) each, at most 64. -> owner[k] for k = 0 .. 63 (None: no staged owner)."""
    owner = [None] * 64
    pm = -1
    for a, (bi, bj) in enumerate(corners):
        K = min(min(i - bi, j - bj), 63) if a >= cur else -1
        prev, pm = pm, max(pm, K)
        for k in range(prev + 1, pm + 1):
            owner[k] = a
    return owner


def owners_search(corners, cur, i, j):
    """the plain rule, cell by cell: the first record from the current one on that holds the cell"""
    owner = [None] * 64
    for k in range(64):
        if k > min(i, j):
            break
        for a in range(cur, len(corners)):
            if i - k >= corners[a][0] and j - k >= corners[a][1]:
                owner[k] = a
                break
    return owner


def owners_walk(corners, cur, i, j):
    """the scalar walk's own stateful form: the current record only advances"""
    owner = [None] * 64
    for k in range(64):
        if k > min(i, j):
            break
        while cur < len(corners) and not (i - k >= corners[cur][0] and j - k >= corners[cur][1]):
            cur += 1
        if cur == len(corners):
            break
        owner[k] = cur
    return owner


def run_length(owner, untraced, i, j):
    """cells the pass may look at: up to the first lane without a staged, traced owner or whose diagonal move would leave the matrix"""
    n = 0
    while n < 64 and n <= min(i, j) - 1 and owner[n] is not None and not untraced[owner[n]]:
        n += 1
    return n


def make_pair(rng):
    n = int(rng.integers(300, 3001))
    ref = synth.rand_str(rng, n, synth.DNA)
    out, pos = [], 0
    events = sorted(rng.integers(0, n, int(rng.integers(3, 40))).tolist())
    for e in events:
        if e < pos:
            continue
        out.append(ref[pos:e])
        kind = rng.integers(0, 6)
        if kind < 2:      # substitution
            out.append(synth.DNA[[(int(np.searchsorted(synth.DNA, ref[e])) + 1) % 4]]); pos = e + 1
        elif kind == 2:   # single-base insertion
            out.append(synth.rand_str(rng, 1, synth.DNA)); pos = e
        elif kind == 3:   # single-base deletion
            pos = e + 1
        elif kind == 4:   # long insertion
            out.append(synth.rand_str(rng, int(rng.integers(20, 201)), synth.DNA)); pos = e
        else:             # long deletion
            pos = min(n, e + int(rng.integers(20, 201)))
    out.append(ref[pos:])
    q = np.concatenate(out)
    return q.astype(np.uint8).tobytes(), ref.astype(np.uint8).tobytes()


def path_cells(cigar, qi, ri):
    cells, i, j = [], qi, ri
    for ln, op in reversed(re.findall(r"(\d+)([MIDX=])", cigar)):
        for _ in range(int(ln)):
            cells.append((i, j))
            i -= op in "M=XI"
            j -= op in "M=XD"
    return cells


def test_running_maximum_finds_the_walks_owner(oracle):
    rng = np.random.default_rng(1111)
    m = S.NucMatrix.new_simple(2, -3)
    checked = crossing4 = grown = with_untraced = dropped = 0
    for p in range(N_PAIRS):
        q, r = make_pair(rng)
        if p % 4 == 0:   # unrelated tails: the X-drop batches' alignments end before them, their stacks with the records of the steps that found no better score
            q += synth.rand_str(rng, 300, synth.DNA).astype(np.uint8).tobytes(); r += synth.rand_str(rng, 300, synth.DNA).astype(np.uint8).tobytes()
        size = SIZES[p % 2]
        mode = ("trace", "x_drop") if p % 4 < 2 else ("trace",)
        x = X_DROP if "x_drop" in mode else 0
        res = oracle.align(m, q, r, GAPS, size, x, mode)
        blocks = oracle.align_blocks(m, q, r, GAPS, size, x, mode)
        # (an alignment that X-drop ended: records beyond its best cell are on the stack, above the record the walk starts in)
        dropped += x > 0 and res["query_idx"] < len(q) and any(row > res["query_idx"] or col > res["reference_idx"] for row, col, _, _ in blocks)
        grown += any(max(w, h) > size[0] for _, _, w, h in blocks)
        stack = [(row, col) for row, col, _, _ in reversed(blocks)]   # from the top, as the walk meets them
        path = path_cells(res["cigar"], res["query_idx"], res["reference_idx"])
        starts = [path[int(x)] for x in rng.integers(0, len(path), 8)] if path else []
        starts += [(int(rng.integers(1, len(q) + 1)), int(rng.integers(1, len(r) + 1))) for _ in range(4)]
        for i, j in starts:
            first = next((a for a, (bi, bj) in enumerate(stack) if i >= bi and j >= bj), None)
            if first is None:
                continue
            top = int(rng.integers(max(0, first - 63), first + 1))     # the staged window: 64 records that include the cell's
            corners = stack[top: top + 64]
            cur = int(rng.integers(0, first - top + 1))
            want = owners_search(corners, cur, i, j)
            assert owners_walk(corners, cur, i, j) == want
            got = owners_model(corners, cur, i, j)
            lim = min(i, j)
            assert got[:lim + 1] == want[:lim + 1], (p, i, j, top, cur)   # (beyond the matrix edge the model may name an owner: those lanes are cut by the edge)
            untraced = rng.random(len(corners)) < (0.05 if p % 5 == 0 else 0.0)
            n = run_length(got, untraced, i, j)
            assert n == run_length(want, untraced, i, j)
            with_untraced += bool(untraced.any()) and n < 64 and want[n] is not None and n <= lim - 1
            crossing4 += len({a for a in want[:lim + 1] if a is not None}) >= 4
            checked += 1
    assert checked > 2000
    assert grown > 10, "no stack with a grown block"
    assert dropped > 10, "no stack with the records of an X-drop end"
    assert with_untraced > 0, "no diagonal was cut by an untraced record"
    assert crossing4 > 0, "no diagonal crosses four records"
