"""What an extension batch and a chain batch refuse after their creation, on the MI355X: the getters before a run, a reload that does not
fit the buffers of the set the batch was created with or has pieces the batch was created without, and a byte outside the alphabet in a
reload. A refused reload leaves the earlier set loaded and served; a failed one leaves nothing loaded until a good one."""
import numpy as np
import pytest

from block_aligner_amd import scores as S

pytestmark = pytest.mark.gpu

NUC = S.NucMatrix.new_simple(2, -3)
GAPS = (-5, -1)
SIZE = (32, 128)
X_DROP = 20
Q0 = b"ACGTTGCAAGGCTTACGATCGATCGGATCCATTGACCAGTAGGCTAACGTTAGCCATGCA"   # 60 bases
R0 = Q0[:13] + b"G" + Q0[14:33] + b"C" + Q0[34:]
Q1 = b"GGATCCTTAGCAGTCAAGCTTGCATGACCGTAGCTAGGAT"                       # 40 bases
R1 = Q1[:5] + b"A" + Q1[6:30] + b"G" + Q1[31:]
Q2 = b"TTGACGGATACCAGTTAGCAAGCTAGCTAGGATCCAGTACGGATCTAGGA"             # 50 bases
R2 = Q2[:25] + b"C" + Q2[26:]


def pool_of(seqs):
    lens = [len(s) for s in seqs]
    off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), off, np.array(lens, np.uint32)


def seeds(seqs, rows):
    """rows: (query, reference, q_seed, r_seed, seed_len) -> ExtendBatchAligner's arrays."""
    pool, off, lens = pool_of(seqs)
    q, r = [c[0] for c in rows], [c[1] for c in rows]
    return (pool, off[q], lens[q], off[r], lens[r]) + tuple(np.array([c[k] for c in rows], np.uint32) for k in (2, 3, 4))


def chains(seqs, rows):
    """rows: (query, reference, [(q_anchor, r_anchor, anchor_len), ...]) -> ChainBatchAligner's arrays."""
    pool, off, lens = pool_of(seqs)
    q, r = [c[0] for c in rows], [c[1] for c in rows]
    first = np.concatenate([[0], np.cumsum([len(c[2]) for c in rows])]).astype(np.uint64)
    anchors = [a for c in rows for a in c[2]]
    return (pool, off[q], lens[q], off[r], lens[r], first) + tuple(np.array([a[k] for a in anchors], np.uint32) for k in (0, 1, 2))


def with_byte(args, at, byte=b"!"):
    pool = args[0].copy()
    pool[at] = ord(byte)
    return (pool,) + args[1:]


def served(b):
    """One run of a traced batch -> (results, (runs, offsets))."""
    b.run()
    res = b.results()
    return res, b.cigars(res["cigar_len"])


def same(a, b):
    (ra, ca), (rb, cb) = a, b
    assert list(ra) == list(rb)
    for k in ra:
        assert np.array_equal(ra[k], rb[k]), k
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1]) and len(ca[0])
    assert not ra["status"].any() and ra["cells"].any()


SEQS = [Q0, R0, Q1, R1, Q2, R2]
SEEDS = [(0, 1, 30, 30, 12), (2, 3, 10, 10, 8), (4, 5, 20, 20, 10)]   # 300 sequence bytes; images of 2 x (16 + 12 + 12) bytes
CHAINS = [(0, 1, [(5, 5, 6), (20, 20, 8), (40, 40, 6)]), (2, 3, [(10, 10, 15)])]   # 200 sequence bytes; images of 2 x (8 + 12 + 8 + 16) bytes


def extend_batch(hip, rows=SEEDS, mode=None, seqs=SEQS):
    return hip.ExtendBatchAligner(NUC, GAPS, SIZE, X_DROP, hip.X_DROP | hip.TRACE if mode is None else mode, *seeds(seqs, rows))


def chain_batch(hip, rows=CHAINS, mode=None, seqs=SEQS[:4]):
    return hip.ChainBatchAligner(NUC, GAPS, SIZE, X_DROP, hip.X_DROP | hip.TRACE if mode is None else mode, *chains(seqs, rows))


def test_extension_getters_before_a_run_and_a_short_buffer(hip):
    eb = extend_batch(hip)
    with pytest.raises(RuntimeError, match="ba_extend_batch_run has not been called"):
        eb.results()
    with pytest.raises(RuntimeError, match="ba_extend_batch_run has not been called"):
        eb.cigars(np.zeros(eb.n, np.uint32))
    res, _ = served(eb)
    total = int(res["cigar_len"].sum())
    short = np.zeros(total - 1, np.uint32)
    assert hip.lib().ba_extend_batch_cigars(eb._h, short.ctypes.data, short.size) != 0
    assert f"cigar buffer too small: need {total} entries" in hip.last_error()
    eb.reload(*seeds(SEQS, SEEDS[:2]))
    with pytest.raises(RuntimeError, match="ba_extend_batch_run has not been called"):
        eb.results()
    eb.close()


@pytest.mark.parametrize("kind", ["extend", "chain"])
def test_cigars_of_an_untraced_batch(hip, kind):
    b = extend_batch(hip, mode=hip.X_DROP) if kind == "extend" else chain_batch(hip, mode=hip.X_DROP)
    for _ in range(2):   # before and after a run
        with pytest.raises(RuntimeError, match="batch was created without BA_TRACE"):
            b.cigars(np.zeros(b.n, np.uint32))
        b.run()
    b.close()


def test_extension_reload_over_capacity(hip):
    eb = extend_batch(hip)
    before = served(eb)
    over = [
        (seeds(SEQS, SEEDS + [(0, 1, 5, 5, 4)]), "reload: 4 seeds exceed the batch's capacity of 3"),
        (seeds(SEQS[:5] + [R2 + b"ACGT"], SEEDS), "reload: 304 sequence bytes exceed the batch's capacity of 300"),
        (seeds(SEQS, [(0, 1, 30, 30, 16)] + SEEDS[1:]), r"reload: the seeds \(88 image bytes\) exceed the batch's capacity of 80"),
    ]
    for args, text in over:
        with pytest.raises(RuntimeError, match=text):
            eb.reload(*args)
        same(served(eb), before)   # the earlier set is still loaded
    eb.close()


def test_chain_reload_over_capacity(hip):
    cb = chain_batch(hip)
    before = served(cb)
    over = [
        (chains(SEQS, CHAINS + [(4, 5, [(20, 20, 10)])]), "reload: 3 chains exceed the batch's capacity of 2"),
        (chains(SEQS[:4], [CHAINS[0], (2, 3, [(5, 5, 5), (20, 20, 10)])]), "reload: 5 anchors exceed the batch's capacity of 4"),
        (chains(SEQS[:3] + [R1 + b"ACGT"], CHAINS), "reload: 204 sequence bytes exceed the batch's capacity of 200"),
        (chains(SEQS[:4], [CHAINS[0], (2, 3, [(10, 10, 20)])]), r"reload: the anchors \(104 image bytes\) exceed the batch's capacity of 88"),
    ]
    for args, text in over:
        with pytest.raises(RuntimeError, match=text):
            cb.reload(*args)
        same(served(cb), before)
    cb.close()


def test_reload_with_pieces_the_batch_was_created_without(hip):
    # every seed covers both of its sequences: no side
    eb = extend_batch(hip, [(0, 0, 0, 0, 60), (3, 3, 0, 0, 40)], seqs=SEQS[:4])
    before = served(eb)
    with pytest.raises(RuntimeError, match="reload: the set has sides to align, and the batch was created with none"):
        eb.reload(*seeds(SEQS[:4], [(0, 1, 30, 30, 12), (2, 3, 10, 10, 8)]))
    after = served(eb)
    assert list(after[0]["score"]) == [120, 80] and not after[0]["cells"].any()
    assert all(np.array_equal(after[0][k], before[0][k]) for k in before[0]) and np.array_equal(after[1][0], before[1][0])
    eb.close()
    # the first anchor starts both sequences and the last one ends them: no end
    cb = chain_batch(hip, [(0, 1, [(0, 0, 6), (20, 20, 8), (50, 50, 10)]), (2, 3, [(0, 0, 10), (25, 25, 15)])])
    before = served(cb)
    with pytest.raises(RuntimeError, match="reload: the set has ends to align, and the batch was created with none"):
        cb.reload(*chains(SEQS[:4], CHAINS))
    same(served(cb), before)
    assert cb.times()["ends_ms"] == 0 and cb.times()["gaps_ms"] > 0
    cb.close()
    # anchors that touch: no gap with two slices to align
    cb = chain_batch(hip, [(0, 1, [(5, 5, 6), (11, 11, 8), (19, 19, 6)]), (2, 3, [(10, 10, 15)])])
    before = served(cb)
    with pytest.raises(RuntimeError, match="reload: the set has gaps to align, and the batch was created with none"):
        cb.reload(*chains(SEQS[:4], CHAINS))
    same(served(cb), before)
    assert cb.times()["gaps_ms"] == 0 and cb.times()["ends_ms"] > 0
    cb.close()


def test_extension_reload_with_a_byte_outside_the_alphabet(hip):
    good = seeds(SEQS, SEEDS)
    fresh = extend_batch(hip)
    want = served(fresh)
    fresh.close()
    eb = extend_batch(hip)
    # inside seed 1 (query 2 at 10 .. 18), inside the right side of seed 2 (reference 5 from 30)
    for at, text in ((120 + 12, "seed 1: byte 0x21 is outside the matrix alphabet"), (200 + 50 + 35, "seed 2: byte 0x21 is outside the matrix alphabet")):
        served(eb)
        with pytest.raises(RuntimeError, match=text):
            eb.reload(*with_byte(good, at))
        with pytest.raises(RuntimeError, match="no seeds loaded"):
            eb.run()
        eb.reload(*good)
        same(served(eb), want)
    eb.close()


def test_chain_reload_with_a_byte_outside_the_alphabet(hip):
    good = chains(SEQS[:4], CHAINS)
    fresh = chain_batch(hip)
    want = served(fresh)
    fresh.close()
    cb = chain_batch(hip)
    # inside anchor 1 of chain 0 (query 0 at 20 .. 28), inside the left end of chain 1 (query 2 before 10),
    # inside the second gap of chain 0 (reference 1 at 28 .. 40)
    for at, text in ((22, "chain 0, anchor 1: byte 0x21 is outside the matrix alphabet"), (120 + 3, "chain 1: byte 0x21 is outside the matrix alphabet"),
                     (60 + 31, "chain 0: byte 0x21 is outside the matrix alphabet")):
        served(cb)
        with pytest.raises(RuntimeError, match=text):
            cb.reload(*with_byte(good, at))
        with pytest.raises(RuntimeError, match="no chains loaded"):
            cb.run()
        cb.reload(*good)
        same(served(cb), want)
    cb.close()
