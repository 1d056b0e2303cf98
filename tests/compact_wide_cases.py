"""Shared by tests/test_compact_wide_gpu.py and tests/test_compact_wide_emu.py: compact keys that also carry the 7-window wide table
(tuning msm_compact = 2) -- the tunables that force the wide flow on sizes the oracle can do, the key's bookkeeping, and the scalars at
the digit boundaries of a half of the split k = k1 + lambda k2."""
import numpy as np

import glv_cases as G

# created and committed under these: msm_compact / msm_wide are read when the key is created, msm_wide_min at every commit
TUNE = dict(msm_compact=2, msm_wide=1, msm_wide_min=0)

# a half is cut into 7 signed 20-bit digits: zero, the tie 0x80000 and its neighbours, a full window, the same in higher windows, and
# 2^64 - 1 (the largest scalar whose k2 is 0)
HALF_VALUES = (0, 1, 2, 0x7FFFF, 0x80000, 0x80001, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, 0x80000 << 20, 0x80001 << 40, 0x7FFFF << 60,
               (1 << 64) - 1)


def compact_wide_key(S, cid, bases, **kw):
    """A key over `bases` created under TUNE, with the bookkeeping every such key must show."""
    with S.tuning(**TUNE):
        ck = S.CommitmentKey(cid, bases, **kw)
    check_bookkeeping(ck, len(bases) if not kw else None)
    return ck


def check_bookkeeping(ck, n):
    assert ck.is_compact() and ck.has_wide_table()
    if n is not None:
        assert ck.table_bytes() == 15 * n * 64, (ck.table_bytes(), n)          # 8 narrow + 7 wide windows of 64-byte points


def boundary_ints(lib, cid, q):
    """Canonical ints: every HALF_VALUES entry x as x (k2 = 0), q - x (a negative half), lambda x (k1 = 0) and q - lambda x; lambda,
    lambda + 1, q - 1, (q +- 1) / 2, 2^253; the scalars with the largest |k1| and |k2| (the top window of a half) and their negatives."""
    lam, _ = G.constants(lib, cid)
    vals = []
    for x in HALF_VALUES:
        vals += [x, (q - x) % q, lam * x % q, (q - lam * x % q) % q]
    vals += [lam, lam + 1, q - 1, (q - 1) // 2, (q + 1) // 2, 1 << 253]
    big1, big2 = G.extreme_scalars(lib, cid, q)
    vals += [big1, big2, q - big1, q - big2]
    return vals


def one_bucket_ints(lib, cid, q):
    """Scalars that, repeated, put every entry into ONE bucket of one segment: zero (no entry at all), +-1, the tie and its neighbour in
    the lowest window of k1, the tie in the lowest window of k2, and the scalar with the largest |k2|."""
    lam, _ = G.constants(lib, cid)
    _, big2 = G.extreme_scalars(lib, cid, q)
    return [0, 1, q - 1, 0x80000, 0x80001, lam * 0x80000 % q, big2]


def commit_counted(ck, v, **kw):
    """ck.commit(v) of a resident / whole vector, asserting that the key counted it as a set outside slot mode."""
    before = ck.msm_stats()["other_sets"]
    got = ck.commit(v, **kw)
    assert ck.msm_stats()["other_sets"] > before
    return got


def dev(a):
    import torch
    return torch.from_numpy(a.view(np.int64)).cuda()
