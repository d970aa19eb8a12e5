"""The end clip (ba_driver.hpp run()) on the Python mirror of the reference's driver: no GPU.

Under X-drop a block that covers both sequence ends is the last one, and all that survives it is best_max and its location. The kernels
therefore stop every rectangle of such a block behind the last residue of its column sequence (width clamp(lenC + 1 - start_j, 0, width):
column lenC holds the last residue, the images being [NULL] + bytes + padding) and set the border
entries the skipped columns of a grow's down part would have written to -32768. The claim: when every matrix entry of the padding byte is
negative, the block's maximum exceeds best_max with the clip iff it does without, and then at the same location.

ClipModel subclasses tests.driver_model.Model and overrides _place: every rectangle of a covering block is placed a second time, clipped, on
copies of the borders -- a grow's right part on the copies its clipped down part left, with the unwritten entries at -32768 -- and the full
and the clipped (max, location) of every rectangle are recorded with best_max at that step. The assertion is per BLOCK (both rectangles of a
grow together, resolved as the driver resolves them: the right part wins ties), because that is the claim: a padding cell of a grow's right
part is strictly below an in-range cell of the block, which may sit in the down part.

best_max is not an attribute of Model (a local of _core): ClipModel re-derives it from what _place returns -- off_max = off + max - ZERO per
step, best_max its running maximum --, with off read back from the rel_zero argument (= ZERO - off; nothing here is near the clamp)."""
import multiprocessing as mp

import numpy as np
import pytest

from block_aligner_amd import scores as S
from block_aligner_amd import synth
from tests.driver_model import L, MIN, STEP, ZERO, Model
from tests.end_clip_pairs import clip_pairs

SIZES = [(32, 256), (128, 512), (128, 1024)]
NUC_GAPS = [(-5, -1), (-4, -2), (-12, -3)]
NEG = -32768


def locate(Dm, ai, aj):
    """(max, row, col) inside the rectangle as the driver reads them: simd_hargmax's first lane at the maximum."""
    mx = int(Dm.max())
    lane = int(np.nonzero(Dm == mx)[0][0])
    return mx, int(ai[lane]) + lane, int(aj[lane])


class ClipModel(Model):
    def __init__(self):
        super().__init__(trace=False, x_drop=True)
        self.records = []       # per covering block: dict(best_max, threshold, full=(mx, where), clip=(mx, where), skipped, rects=[...])
        self._best = 0
        self._step = None       # the step in flight: (off, [maxima of its rectangles])
        self._shadow = None     # clipped copies of the four borders between the two rectangles of a covering grow
        self._block = None

    def _finish_step(self):
        if self._step is not None:
            off, maxima = self._step
            self._best = max(self._best, off + max(maxima) - ZERO)
            self._step = None
        if self._block is not None:
            self._close_block()

    def _close_block(self):
        b, self._block = self._block, None
        # a grow: the right part (last) wins ties over the down part, as scan_block.rs:370-404 resolves them
        def resolve(key):
            rects = b["rects"]
            mx, where = rects[-1][key][0], ("last",) + rects[-1][key][1:]
            if len(rects) == 2 and rects[0][key][0] > mx:
                mx, where = rects[0][key][0], ("first",) + rects[0][key][1:]
            return mx, where
        b["full"], b["clip"] = resolve("full"), resolve("clip")
        self.records.append(b)

    def _place(self, seqv, lenv, seqc, lenc, start_i, start_j, width, height, Dc, Cc, Dr, Rr, corner, rel_zero, right):
        shift = Dr is self.temp1
        grow_down = not shift and not right
        if shift or grow_down:
            self._finish_step()
            self._step = (ZERO - rel_zero, [MIN])
        if self._step is None:          # (the right part of the very first grow: its down part has height 0 and is not a call worth the name)
            self._step = (ZERO - rel_zero, [MIN])
        # the block this rectangle belongs to, from the rectangle (scan_block.rs:160-305)
        if shift:
            bs = height
            si, sj = (start_i, start_j - (bs - STEP)) if right else (start_j - (bs - STEP), start_i)
        elif right:
            bs = height
            si, sj = start_i, start_j - (bs - width)
        else:
            bs = width + height
            si, sj = start_j - height, start_i
        covers = si + bs > self.qlen and sj + bs > self.rlen
        if covers and width > 0 and height > 0:
            wc = min(max(lenc + 1 - start_j, 0), width)   # (column lenc is the last residue: PaddedBytes are [NULL] + bytes + padding)
            if grow_down:
                self._shadow = [a.copy() for a in (self.D_col, self.C_col, self.D_row, self.R_row)]
                sD, sC, sDr, sRr = self._shadow[2], self._shadow[3], self._shadow[0][height:], self._shadow[1][height:]
            elif not shift and self._shadow is not None:
                prev = bs - width
                sD, sC, sDr, sRr = self._shadow[0], self._shadow[1], self._shadow[2][prev:], self._shadow[3][prev:]
            else:
                sD, sC, sDr, sRr = Dc.copy(), Cc.copy(), Dr.copy(), Rr.copy()
            cells = self.cells
            clip = locate(*Model._place(self, seqv, lenv, seqc, lenc, start_i, start_j, wc, height, sD, sC, sDr, sRr, corner, rel_zero, right))
            self.cells = cells
            if grow_down:
                sDr[wc:width] = NEG; sRr[wc:width] = NEG
            else:
                self._shadow = None
        out = Model._place(self, seqv, lenv, seqc, lenc, start_i, start_j, width, height, Dc, Cc, Dr, Rr, corner, rel_zero, right)
        self._step[1].append(int(out[0].max()))
        if covers and width > 0 and height > 0:
            if self._block is None:
                # (the driver compares off + max - ZERO with best_max: as a raw cell value of this step's offset base the threshold is
                # best_max - off + ZERO = best_max + rel_zero)
                self._block = dict(best_max=self._best, threshold=self._best + rel_zero, skipped=0, rects=[], size=bs)
            self._block["rects"].append(dict(full=locate(*out), clip=clip, width=width, clipped_width=wc, height=height, right=right))
            self._block["skipped"] += (width - wc) * height
        return out

    def align(self, *a, **k):
        out = super().align(*a, **k)
        self._finish_step()
        return out


def run_chunk(args):
    kind, seed, count = args
    alpha = synth.DNA if kind == "nuc" else synth.AMINO
    pairs = clip_pairs(count, alpha, seed)
    rng = np.random.default_rng(seed + 1)
    n_blocks = n_clipped = n_new_best = 0
    bad = []
    for p, (q, r) in enumerate(pairs):
        size = SIZES[p % len(SIZES)]
        if kind == "nuc":
            matrix, gaps = S.NucMatrix.new_simple(2, -3), NUC_GAPS[(p // len(SIZES)) % len(NUC_GAPS)]
        else:
            matrix, gaps = S.static_matrix("BLOSUM62"), (-11, -1)
        m = ClipModel()
        m.align(q, r, matrix, gaps, size, int(rng.integers(60, 300)))
        clipped_pair = False
        for b in m.records:
            n_blocks += 1
            clipped_pair |= b["skipped"] > 0
            full_new, clip_new = b["full"][0] > b["threshold"], b["clip"][0] > b["threshold"]
            n_new_best += full_new
            if full_new != clip_new or (full_new and b["full"] != b["clip"]):
                bad.append((kind, seed, p, size, gaps, b))
        n_clipped += clipped_pair
    return len(pairs), n_clipped, n_blocks, n_new_best, bad


def run_all(kind, total, seed0, workers=8, per=50):
    jobs = [(kind, seed0 + 7 * k, min(per, total - k * per)) for k in range((total + per - 1) // per)]
    with mp.get_context("fork").Pool(workers) as pool:
        return pool.map(run_chunk, jobs)


@pytest.mark.parametrize("kind,total", [("nuc", 2000), ("aa", 500)])
def test_clipped_last_block_agrees_with_the_full_one(kind, total):
    """2000 DNA pairs (new_simple(2, -3); gaps (-5, -1), (-4, -2), (-12, -3)) and 500 protein pairs (BLOSUM62, (-11, -1)) of 100..900 residues
    with independent tails of 0..600, every fifth with one 100..400 residue indel in its last 500, at (32, 256), (128, 512) and (128, 1024),
    X-drop 60..299 (a small X-drop ends most of these alignments inside the tail, before any block reaches both ends; a large one lets the
    closing grows run). At least a quarter of the pairs must end in a block that has something to clip."""
    out = run_all(kind, total, 4100 if kind == "nuc" else 9100)
    pairs = sum(o[0] for o in out); clipped = sum(o[1] for o in out); blocks = sum(o[2] for o in out); new_best = sum(o[3] for o in out)
    bad = [b for o in out for b in o[4]]
    print(f"{kind}: {pairs} pairs, {clipped} with a clipped last block, {blocks} covering blocks, {new_best} of them raise the best")
    assert pairs == total
    assert clipped * 4 >= pairs, (clipped, pairs)
    assert not bad, bad[:3]


def test_a_non_negative_padding_score_breaks_the_premise():
    """A NucMatrix that scores 'Z' (the padding byte) against 'A' at +1: padding columns can now gain, so the lemma's premise fails and the
    host leaves F_PAD_NEG clear for such a matrix (ba_host.cpp pad_negative). This case only documents that: the model runs, the full and the
    clipped maxima are printed, nothing is asserted about their equality."""
    m = S.NucMatrix.new_simple(2, -3)
    m.set(ord("Z"), ord("A"), 1)
    raw = np.asarray(m.raw(), np.int64).ravel()
    assert raw[(ord("Z") & 7) * 16 + (ord("A") & 15)] == 1 and raw[(ord("A") & 7) * 16 + (ord("Z") & 15)] == 1
    differ = blocks = 0
    for q, r in clip_pairs(40, synth.DNA, 77):
        cm = ClipModel()
        cm.align(q, r, m, (-5, -1), (128, 1024), 60)
        for b in cm.records:
            blocks += 1
            differ += b["full"][0] != b["clip"][0]
    print(f"padding scored +1 against 'A': {differ} of {blocks} covering blocks have another maximum when clipped")
    assert blocks > 0
