"""The seeding model itself, without a GPU: the known answers of INTEGRATION.md, "Seeding", the hash, the plain and the NumPy statement of the
rule against one another, w = 1 against a brute-force enumeration, the window guarantee, the order of the hits, and that the model's hits on
the chain sets of the GPU pipeline test leave no read without a chain."""
import numpy as np
import pytest

from tests import chain_ref, chaining_ref, seeding_ref as S


def test_hash_check_values():
    for x, h in S.HASH_CHECKS.items():
        assert S.h32(x) == h, hex(x)
    xs = np.array(list(S.HASH_CHECKS), np.uint64)
    assert S.h32_np(xs).tolist() == list(S.HASH_CHECKS.values())


def test_hash_is_a_bijection_on_a_sample():
    xs = np.arange(1 << 16, dtype=np.uint64) * np.uint64(65521)
    assert len(np.unique(S.h32_np(xs & np.uint64(S.MASK)))) == 1 << 16


def test_first_known_answer():
    assert S.sketch_plain(S.KNOWN_Q, 5, 4)[0] == S.KNOWN_Q_SKETCH
    assert S.sketch_plain(S.KNOWN_R, 5, 4)[0] == S.KNOWN_R_SKETCH
    assert S.hits_plain(S.KNOWN_Q, S.KNOWN_R, S.Params(5, 4, 2)) == S.KNOWN_HITS_OCC2
    assert S.hits_plain(S.KNOWN_Q, S.KNOWN_R, S.Params(5, 4, 1)) == S.KNOWN_HITS_OCC1
    for occ, want in ((2, S.KNOWN_HITS_OCC2), (1, S.KNOWN_HITS_OCC1)):
        e = S.hits(S.KNOWN_Q, S.KNOWN_R, S.Params(5, 4, occ))
        assert e["q_pos"].tolist() == S.KNOWN_Q_SKETCH and e["r_pos"].tolist() == S.KNOWN_R_SKETCH
        assert list(zip(e["q_hit"].tolist(), e["r_hit"].tolist())) == want


def test_second_known_answer_on_the_minus_strand():
    P = S.Params(5, 3, 4)
    assert S.sketch_plain(S.oriented(S.KNOWN_Q_MINUS, 1), 5, 3)[0] == S.KNOWN_Q_MINUS_SKETCH
    assert S.hits_plain(S.KNOWN_Q_MINUS, S.KNOWN_R, P, 1) == S.KNOWN_HITS_MINUS
    e = S.hits(S.KNOWN_Q_MINUS, S.KNOWN_R, P, 1)
    assert e["q_pos"].tolist() == S.KNOWN_Q_MINUS_SKETCH
    assert list(zip(e["q_hit"].tolist(), e["r_hit"].tolist())) == S.KNOWN_HITS_MINUS


def test_the_strand_frame():
    assert S.oriented(b"acgTNn-x", 1) == b"X-NNACGT"
    assert S.oriented(b"acgTNn-x", 0) == b"acgTNn-x"
    assert S.oriented(b"ACCGT", 1) == chain_ref.revcomp(b"ACCGT")


def _small_sets():
    return [S.lengths_set(4, 2), S.lengths_set(15, 16), S.other_bytes_set(5, 4), S.tie_set(), S.occ_set(6, 3), S.strand_set()]


def test_plain_and_numpy_statements_agree():
    for ps, P in zip(_small_sets(), (S.Params(4, 2, 3), S.Params(15, 16, 2), S.Params(5, 4, 2), S.Params(4, 7, 1000), S.Params(6, 1, 3), S.Params(8, 5, 4))):
        for (q, r, s), e in zip(ps.pairs, ps.expected(P)):
            assert S.sketch_plain(S.oriented(q, s), P.k, P.w) == (e["q_pos"].tolist(), e["q_code"].tolist())
            assert S.sketch_plain(r, P.k, P.w) == (e["r_pos"].tolist(), e["r_code"].tolist())
            assert S.hits_plain(q, r, P, s) == list(zip(e["q_hit"].tolist(), e["r_hit"].tolist()))


def test_the_largest_code_matches_like_any_other():
    """The all-T 16-mer has the code 0xffffffff: the end of its run among the sorted keys is not found by searching for code + 1."""
    P = S.Params(16, 64, 1000)
    for (q, r, s), e in zip(S.tie_set().pairs, S.tie_set().expected(P)):
        assert S.hits_plain(q, r, P, s) == list(zip(e["q_hit"].tolist(), e["r_hit"].tolist()))
    e = S.hits(b"A" * 300, b"T" * 300, P, 1)
    assert set(e["r_code"].tolist()) == {0xffffffff} and len(e["q_hit"]) == 222 * 222


def test_w_1_without_a_cap_is_every_shared_kmer():
    n_hits = 0
    for ps, k in ((S.lengths_set(4, 1), 4), (S.other_bytes_set(6, 1), 6), (S.strand_set(), 9), (S.tie_set(), 5)):
        for q, r, s in ps.pairs:
            got = S.hits(q, r, S.Params(k, 1, S.NO_CAP), s)
            want = S.brute_force_hits(q, r, k, s)
            assert list(zip(got["q_hit"].tolist(), got["r_hit"].tolist())) == want
            n_hits += len(want)
    assert n_hits > 10000


def test_every_window_with_a_valid_kmer_holds_a_selected_position():
    checked = 0
    for ps, (k, w) in zip((S.lengths_set(4, 16), S.other_bytes_set(5, 4), S.tie_set(), S.strand_set()), ((4, 16), (5, 4), (4, 7), (8, 5))):
        for q, r, s in ps.pairs:
            for seq in (S.oriented(q, s), r):
                cs = S.codes_plain(seq, k)
                pos = set(S.sketch(seq, k, w)[0].tolist())
                assert all(cs[i] is not None for i in pos)
                nk = len(cs)
                for a in range(max(1, nk - w + 1) if nk else 0):
                    win = range(a, min(a + w, nk))
                    if any(cs[i] is not None for i in win):
                        assert any(i in pos for i in win), (a, k, w)
                        checked += 1
    assert checked > 5000


def test_hits_are_sorted_and_a_chaining_problem_set_keeps_their_order():
    for ps, P in ((S.strand_set(), S.Params(8, 5, 4)), (S.tie_set(), S.Params(4, 7, 1000)), (S.occ_set(6, 3), S.Params(6, 1, 3))):
        exp = ps.expected(P)
        cps = chaining_ref.ProblemSet([(e["q_hit"], e["r_hit"], np.full(len(e["q_hit"]), P.k)) for e in exp])
        for e, (q, r, L) in zip(exp, cps.problems):
            pairs = list(zip(e["r_hit"].tolist(), e["q_hit"].tolist()))
            assert pairs == sorted(pairs) and len(set(pairs)) == len(pairs)
            assert q.tolist() == e["q_hit"].tolist() and r.tolist() == e["r_hit"].tolist()
            assert (e["q_hit"].astype(np.int64) + P.k <= (1 << 31)).all()


def test_the_sets_of_the_gpu_tests_hold_what_they_are_for():
    """The sort set's queries have SORT_ENTRIES selected entries with w = 1 and duplicated codes; the occurrence set sits on the cap; the
    over-limit set counts more than 2^28."""
    ss = S.sort_set()
    for (q, r, _), n in zip(ss.pairs, S.SORT_ENTRIES):
        pos, code = S.sketch(q, 15, 1)
        assert len(pos) == n
        if n >= 200:
            assert len(np.unique(code)) < n
    k, occ = 6, 3
    ps = S.occ_set(k, occ)
    e = ps.expected(S.Params(k, 1, occ))
    counts = [np.unique(x["q_code"], return_counts=True)[1].max() for x in e]
    assert counts[0] == occ and counts[1] == occ + 1
    assert len(e[0]["q_hit"]) >= 2 * occ and len(e[2]["q_hit"]) >= 2 * occ
    capped = S.hits(*ps.pairs[1][:2], S.Params(k, 1, occ))
    free = S.hits(*ps.pairs[1][:2], S.Params(k, 1, occ + 1))
    assert len(free["q_hit"]) == len(capped["q_hit"]) + occ + 1
    assert (17000 - 15 + 1) ** 2 > 1 << 28


@pytest.mark.parametrize("name", ["minus", "mixed"])
def test_seeding_the_chain_sets_leaves_no_read_without_a_chain(name):
    """What the GPU pipeline test relies on: the model's hits (k 10, w 5, max_occ 8) of every read of the set, chained by the chaining model
    with E2E_PARAMS, give every read at least one chain."""
    cs = chain_ref.dna_sets()[name]
    P = S.PIPELINE_PARAMS
    _, pairs = S.chain_set_problems(cs)
    without, fewest, most = 0, None, 0
    for q, r, s in pairs:
        e = S.hits(q, r, P, s)
        n = len(e["q_hit"])
        fewest, most = n if fewest is None else min(fewest, n), max(most, n)
        res = chaining_ref.chain(chaining_ref.E2E_PARAMS, e["q_hit"], e["r_hit"], [P.k] * n)
        without += not res["chains"]
    assert without == 0, (without, len(pairs), fewest, most)
