"""The model of tests/select_ref.py (the rule of INTEGRATION.md, "Selecting a read's alignments") on the CPU: the known answer, the
properties the rule promises on random sets, and what the sets of the GPU tests are meant to hold."""
import numpy as np
import pytest

from tests import select_ref as R


def test_the_known_answer():
    out = R.known_set().expected(R.KNOWN_PARAMS)
    for k, v in R.KNOWN_OUT.items():
        assert out[k] == v, k


def test_the_known_answer_holds_what_the_chapter_says():
    K = R.KNOWN
    # candidate 2, mirrored: [480, 980) against candidate 1's [0, 500): 20 of 500 bases, below half -> a head of its own
    assert (K["q_len"][2] - K["q_end"][2], K["q_len"][2] - K["q_start"][2]) == (480, 980)
    assert 1000 * 20 < R.KNOWN_PARAMS.mask_permille * 500
    # candidate 0 under candidate 2: 300 < 0.8 * 480
    assert 1000 * 300 < R.KNOWN_PARAMS.sec_permille * 480
    # candidates 7 and 9 tie: the lower index is the primary, and s1 == s2 gives mapq 0
    assert K["score"][7] == K["score"][9] and R.KNOWN_OUT["mapq"][7] == 0


def random_set(seed, distinct=False):
    rng = np.random.default_rng(seed)
    rows = [row for r in range(12) for row in R.random_read(rng, r, int(rng.integers(0, 60)), distinct_scores=distinct, low=0.0 if distinct else 0.1)]
    return R.from_rows(rows, 12, rng)


@pytest.mark.parametrize("seed", range(6))
def test_properties_on_random_sets(seed):
    rng = np.random.default_rng(100 + seed)
    P = R.Params(int(rng.integers(1, 1001)), int(rng.integers(0, 1001)), int(rng.integers(0, 6)), int(rng.integers(0, 256)), int(rng.integers(1, 30)), 20)
    cs = random_set(seed)
    out = cs.expected(P)
    n = len(cs)
    heads = [c for c in range(n) if out["cls"][c] <= R.SUPPLEMENTARY]
    for r in range(cs.n_reads):
        mine = [c for c in range(n) if cs.read[c] == r and out["cls"][c] != R.EXCLUDED]
        prim = [c for c in mine if out["cls"][c] == R.PRIMARY]
        assert len(prim) == (1 if mine else 0) and all(out["rank"][c] == 0 for c in prim), r   # exactly one primary, at rank 0
        assert sorted(out["rank"][c] for c in mine) == list(range(len(mine)))
        kept = out["kept"][out["kept_first"][r]:out["kept_first"][r + 1]]
        my_heads = [c for c in mine if c in heads]
        assert len(kept) <= len(my_heads) + P.max_secondary and len(kept) == out["kept_per_read"][r]
        assert [out["rank"][c] for c in kept] == sorted(out["rank"][c] for c in kept) and all(out["cls"][c] <= R.SECONDARY for c in kept)
    for c in range(n):
        if out["cls"][c] == R.EXCLUDED:
            assert (out["parent"][c], out["rank"][c], out["mapq"][c], out["sub_score"][c]) == (R.NONE, R.NONE, 0, 0)
            continue
        p = out["parent"][c]
        assert p in heads and cs.read[p] == cs.read[c], c                        # every parent is a head of the same read
        assert (p == c) == (c in heads)
        assert out["mapq"][c] <= P.mapq_max and out["sub_score"][c] <= cs.score[c]
        if c not in heads:
            assert out["mapq"][c] == 0 and out["sub_score"][c] == 0 and cs.score[c] <= out["sub_score"][p] <= cs.score[p]


@pytest.mark.parametrize("seed", range(4))
def test_the_callers_order_does_not_matter_without_score_ties(seed):
    cs = random_set(50 + seed, distinct=True)
    for r in range(cs.n_reads):   # (no two eligible candidates of a read share a score)
        s = [int(cs.score[c]) for c in range(len(cs)) if cs.read[c] == r and cs.score[c] >= 20]
        assert len(s) == len(set(s))
    P = R.GPU_PARAMS
    out = cs.expected(P)
    perm = np.random.default_rng(seed).permutation(len(cs))   # new position k holds old candidate perm[k]
    inv = np.argsort(perm)
    got = cs.permuted(perm).expected(P)
    back = lambda c: c if c == R.NONE else int(perm[c])
    for k in ("cls", "mapq", "rank", "sub_score"):
        assert [got[k][inv[c]] for c in range(len(cs))] == out[k], k
    assert [back(got["parent"][inv[c]]) for c in range(len(cs))] == out["parent"]
    assert [back(c) for c in got["kept"]] == out["kept"] and got["kept_first"] == out["kept_first"]


def test_the_gpu_sets_hold_what_their_tests_are_about():
    sets = R.gpu_sets()
    P = R.GPU_PARAMS
    sizes = sets["sizes"]
    assert np.bincount(sizes.read, minlength=len(R.SIZES)).tolist() == list(R.SIZES) and max(R.SIZES) == R.MAX_PER_READ
    assert sizes.read.tolist() != sorted(sizes.read.tolist())   # shuffled caller order
    out = sizes.expected(P)
    heads_of = lambda o, cs, r: sum(1 for c in range(len(cs)) if cs.read[c] == r and o["cls"][c] <= R.SUPPLEMENTARY)
    assert heads_of(out, sizes, len(R.SIZES) - 1) > 64        # a second chunk of heads
    assert set(out["cls"]) == {0, 1, 2, 3, 4}
    special = sets["special"]
    out = special.expected(P)
    assert heads_of(out, special, 0) == 130                    # three 64-head steps
    tie = [c for c in range(len(special)) if special.read[c] == 1 and out["cls"][c] != R.EXCLUDED]
    assert len(tie) > 64 and len({int(special.score[c]) for c in tie}) == 1 and sorted(tie, key=lambda c: out["rank"][c]) == tie
    assert all(out["cls"][c] == R.EXCLUDED for c in range(len(special)) if special.read[c] == 2) and out["kept_per_read"][2] == 0
    assert any(int(s) > P.full_support for s in special.support) and any(int(s) < P.full_support for s in special.support)
    many = sets["many"]
    assert many.n_reads == 3000 and set(np.bincount(many.read, minlength=3000).tolist()) == {1, 2, 3, 4}
    assert len(sets["smaller"]) < len(sizes) and sets["smaller"].n_reads <= sizes.n_reads
    for ms in R.MAX_SECONDARY:   # the cap binds, and is lifted
        o = sizes.expected(P._replace(max_secondary=ms))
        assert max(sum(1 for c in o["kept"][o["kept_first"][r]:o["kept_first"][r + 1]] if o["cls"][c] == R.SECONDARY) for r in range(sizes.n_reads)) <= ms
    assert sizes.expected(P._replace(max_secondary=0))["cls"] != sizes.expected(P._replace(max_secondary=64))["cls"]
    assert sizes.expected(P._replace(mask_permille=1))["cls"] != sizes.expected(P._replace(mask_permille=1000))["cls"]
    assert sizes.expected(P._replace(sec_permille=0))["cls"] != sizes.expected(P._replace(sec_permille=1000))["cls"]
    assert sizes.expected(P)["mapq"] != sizes.replace(support=None).expected(P)["mapq"]
