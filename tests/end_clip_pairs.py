"""Pairs for the end-clip tests (tests/test_end_clip_model.py, tests/test_gpu_end_clip.py): alignments whose last block reaches past both
sequence ends by very different amounts.

A pair is a common core (the query a lightly mutated copy of it), optionally one long insertion or deletion in the core's last 500 residues,
and then an unrelated random tail on EACH sequence, the two tail lengths drawn independently from the same range -- so one sequence often
ends hundreds of residues before the other ("ragged"), and with X-drop the alignment ends near the end of the core: the checkpoint the closing
grows start from lies 0 .. 600 positions before either end, on both sides of 128, 256 and 512."""
import numpy as np

from block_aligner_amd import synth


def clip_pair(rng, alphabet, length=(100, 900), tail=(0, 600), indel=False, sub_rate=0.03):
    n = int(rng.integers(length[0], length[1] + 1))
    core = synth.rand_str(rng, n, alphabet)
    q = synth.mutate(rng, core, int(n * sub_rate), alphabet)
    r = core
    if indel:   # one 100 .. 400 residue event in the last 500 residues, in either sequence
        k = int(rng.integers(100, 401))
        at = int(rng.integers(max(0, n - 500), n + 1))
        ins = synth.rand_str(rng, k, alphabet)
        if rng.integers(0, 2):
            q = np.concatenate([q[:at], ins, q[at:]])
        else:
            r = np.concatenate([r[:at], ins, r[at:]])
    tq, tr = (int(x) for x in rng.integers(tail[0], tail[1] + 1, 2))
    if rng.integers(0, 4) == 0:   # every fourth pair: one sequence ends with the core
        if rng.integers(0, 2):
            tq = 0
        else:
            tr = 0
    q = np.concatenate([q, synth.rand_str(rng, tq, alphabet)])
    r = np.concatenate([r, synth.rand_str(rng, tr, alphabet)])
    return q.astype(np.uint8).tobytes(), r.astype(np.uint8).tobytes()


def clip_pairs(n, alphabet, seed, length=(100, 900), tail=(0, 600), indel_every=5):
    rng = np.random.default_rng(seed)
    return [clip_pair(rng, alphabet, length, tail, indel=indel_every > 0 and p % indel_every == 0) for p in range(n)]
