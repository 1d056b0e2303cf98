"""Shared by tests/test_plain_batch_gpu.py and tests/test_plain_batch_emu.py: sets of MSMs on plain commitment keys (tuning msm_plain = 1 or
2) that run as ONE linked flow, the (member, window) pairs of the set as its segments -- the batch counted through plain_batch_stats(),
plain_stats() and msm_stats(), and the member lengths at which the flat tile space, the segment index or the landing offset can go wrong.
Every result is compared with the oracle's MSM of the vector over the key's prefix, bit for bit."""
import numpy as np

import plain_fold_cases as PF

KEYS = [(0, 1), (1, 2)]           # (curve, form): form 1 on bn256, form 2 on grumpkin
CROSSED = [(0, 2), (1, 1)]        # the two other pairs, for the shapes
KEY_N = 3000

# member lengths -> (sets, msms) that plain_batch_stats() must rise by.  WIDE_TILE = 512 scalars per workgroup of the segment passes.
SHAPES = {
    "tiles": ((513, 0, 1, 512, 3000), (1, 4)),        # one scalar past a tile, an empty member in the middle, one exactly-full tile
    "empty": ((0, 0, 0), (0, 0)),                     # nothing launched, three identities
    "single": ((5,), (0, 0)),                         # one member: the sequential path
    "sixteen": (tuple(range(1, 17)), (1, 16)),        # S = 256 segments on form 1
    "seventeen": (tuple(range(1, 18)), (1, 16)),      # cut into sets of 16 and 1
}


def batch_key(S, cid, form, bases):
    return PF.fold_key(S, cid, form, bases)


def counted(ck, run, sets, msms, reductions):
    """run(), asserting what the key counted meanwhile: sets that ran the batched flow, the MSMs they carried, bucket reductions of the
    plain flow (one per non-empty member, batched or not) -- and that nothing folded or went anywhere but the plain flow."""
    b0, p0 = ck.plain_batch_stats(), ck.plain_stats()
    got = run()
    b1, p1, m1 = ck.plain_batch_stats(), ck.plain_stats(), ck.msm_stats()
    assert (b1["sets"] - b0["sets"], b1["msms"] - b0["msms"]) == (sets, msms), (b0, b1)
    assert (p1["fold_sets"] - p0["fold_sets"], p1["reductions"] - p0["reductions"]) == (0, reductions), (p0, p1)
    assert (m1["slot_sets"], m1["hot_sets"], m1["redo"]) == (0, 0, 0), m1
    return got


def oracle_batch(O, cid, vs, bases):
    return np.stack([O.msm(cid, v, bases[:len(v)]) if len(v) else np.zeros(8, np.uint64) for v in vs])


def member_vectors(O, cid, lens, seed):
    """(n, 4) Montgomery scalars per member: uniform and trace-like in turn"""
    from conftest import seeded_scalars
    return [seeded_scalars(O, cid, n, seed + 7 * j, "trace" if j % 2 else "uniform") if n else np.zeros((0, 4), np.uint64)
            for j, n in enumerate(lens)]


def mont(O, cid, ints):
    return O.ints_to_mont(O.SCALAR_FIELD[cid], list(ints))
