"""The models of tests/index_ref.py against tests/seeding_ref.py and against answers worked out by hand (no GPU): the indexed rule without a
reference cap is the plain rule, the cap counts occurrences in the reference's sketch, the candidate windows, and the read set of the whole
path, whose every read the models alone place where it was drawn from."""
import numpy as np
import pytest

from tests import chain_ref, index_ref as X, seeding_ref as S
from tests.test_gpu_chain import DNA_GAPS, NUC, X_DROP


def pairs(e):
    return list(zip(e["q_hit"].tolist(), e["r_hit"].tolist()))


def test_without_a_reference_cap_the_indexed_rule_is_the_plain_rule():
    for q, strand, k, w, occ, want in ((S.KNOWN_Q, 0, 5, 4, 2, S.KNOWN_HITS_OCC2), (S.KNOWN_Q, 0, 5, 4, 1, S.KNOWN_HITS_OCC1),
                                       (S.KNOWN_Q_MINUS, 1, 5, 3, 4, S.KNOWN_HITS_MINUS)):
        P = X.Params(k, w, occ, X.NO_CAP)
        assert pairs(X.hits(q, S.KNOWN_R, P, strand)) == want
        assert X.hits_plain(q, S.KNOWN_R, P, strand) == want
    rng = np.random.default_rng(3)
    ref = S.dna(rng, 3000)
    for strand in (0, 1):
        read = S.oriented(S.mutate(rng, ref[700:1500], 0.05), strand)
        P = X.Params(8, 4, 3, X.NO_CAP)
        e = S.hits(read, ref, S.Params(8, 4, 3), strand)
        assert pairs(X.hits(read, ref, P, strand)) == pairs(e) == X.hits_plain(read, ref, P, strand) and len(e["q_hit"]) > 50


def test_the_entries_are_the_sketch_sorted_by_code_and_position():
    code, pos, longest = X.entries(S.KNOWN_R, 5, 4)
    assert sorted(pos.tolist()) == S.KNOWN_R_SKETCH
    assert list(zip(code.tolist(), pos.tolist())) == sorted(zip(code.tolist(), pos.tolist()))
    cs = S.codes_plain(S.KNOWN_R, 5)
    assert code.tolist() == [cs[j] for j in pos.tolist()]
    assert longest == 2   # TTGCA is selected at 5 and at 31 (the hits (3, 5) and (3, 31) of the known answers); every other code once
    assert X.entries(b"ACG", 5, 4)[2] == 0 and len(X.entries(b"ACG", 5, 4)[0]) == 0


@pytest.mark.parametrize("max_occ, max_ref_occ", [(1, 1), (2, 3), (3, 2)])
def test_the_reference_cap_at_the_cap_and_one_over(max_occ, max_ref_occ):
    """occ_case's four k-mers: hits only from the one that stays within both caps, max_occ * max_ref_occ of them."""
    k = 13
    ref, rs = X.occ_case(k, max_occ, max_ref_occ)
    P = X.Params(k, 1, max_occ, max_ref_occ)
    read, strand = rs.reads[0]
    free = S.brute_force_hits(read, ref, k, strand)
    got = pairs(X.hits(read, ref, P, strand))
    assert got == X.hits_plain(read, ref, P, strand)
    assert len(got) == max_occ * max_ref_occ
    assert len(free) == len(got) + (max_ref_occ + 1) * max_occ + max_ref_occ * (max_occ + 1) + (max_ref_occ + 1) * (max_occ + 1)
    one_more = pairs(X.hits(read, ref, P._replace(max_ref_occ=max_ref_occ + 1), strand))   # ... lets every k-mer of the reference through
    assert one_more == pairs(S.hits(read, ref, S.Params(k, 1, max_occ), strand)) and len(one_more) == (2 * max_ref_occ + 1) * max_occ
    assert pairs(X.hits(*rs.reads[1][:1], ref, P, 1)) == got          # the same read given as its reverse complement


def test_windows_by_hand():
    """One reference of 1000 bases at offset 5000, reads of 100 bases, margin 10."""
    q_len, r_off, r_len = [100] * 4, [5000] * 4, [1000] * 4
    chains = [[(20, 5, 10), (40, 26, 10)],       # at the reference's start: qa0 + margin = 30 > ra0 = 5 -> lo = 0; hi = 36 + (50 + 10) = 96
              [(10, 900, 10), (60, 960, 20)],    # at its end: lo = 900 - 20 = 880; re = 980, r_len - re = 20 < 20 + 10 -> hi = 1000
              [(30, 500, 10), (50, 520, 30)],    # clipped by the margin on both sides: lo = 500 - 40 = 460; hi = 550 + (20 + 10) = 580
              [(0, 300, 100)]]                   # one anchor over the whole read: lo = 300 - 10 = 290; hi = 400 + 10 = 410
    first = np.concatenate([[0], np.cumsum([len(c) for c in chains])])
    flat = [a for c in chains for a in c]
    r_off_w, r_len_w, r_anchor_w, shift = X.chain_windows(q_len, r_off, r_len, first, [a[0] for a in flat], [a[1] for a in flat], [a[2] for a in flat], 10)
    assert shift.tolist() == [0, 880, 460, 290]
    assert r_off_w.tolist() == [5000, 5880, 5460, 5290]
    assert r_len_w.tolist() == [96, 120, 120, 120]
    assert r_anchor_w.tolist() == [5, 26, 20, 80, 40, 60, 10]
    with pytest.raises(ValueError, match="chain 1 has no anchors"):
        X.chain_windows([100, 100], [0, 0], [1000, 1000], [0, 1, 1], [0], [0], [10], 10)
    with pytest.raises(ValueError, match="chain 0: anchor 1 ends outside its sequences"):
        X.chain_windows([100], [0], [1000], [0, 2], [0, 95], [0, 200], [10, 10], 10)


def test_the_models_place_every_read_where_it_was_drawn_from(oracle):
    """The whole path in the models: hits, chains, windows, chain alignment. For every read, the rank-0 chain on its true strand, shifted
    back, overlaps the interval the read was drawn from: what tests/test_gpu_index.py asserts of the device."""
    ms = X.MappingSet()
    assert len(ms.reads) == 80 and sum(s for _, _, s in ms.origin) == 20
    exps = ms.reads.expected(ms.ref, X.MAP_PARAMS)
    chains = X.model_chains(ms, exps)
    cs, shift = X.windowed_chain_set(ms, chains)
    assert len(cs) <= 300
    piece = chain_ref.oracle_piece(oracle, NUC, DNA_GAPS, (32, 256), X_DROP, True, True)
    at = {(p, rank): c for c, (p, rank, _) in enumerate(chains)}
    for i in range(len(ms.origin)):
        c = at.get((ms.true_problem(i), 0))
        assert c is not None, i
        res = chain_ref.chain_result(piece, NUC, DNA_GAPS, cs.q(c), cs.r(c), cs.anchors(c), True, True)
        assert res["status"] == 0
        lo, hi = res["r_start"] + int(shift[c]), res["r_end"] + int(shift[c])
        assert X.overlaps_origin(ms, i, lo, hi), (i, lo, hi, ms.origin[i])
        a, b, _ = ms.origin[i]
        assert min(hi, b) - max(lo, a) >= (b - a) // 2   # (not by a base: at least half of the interval)
