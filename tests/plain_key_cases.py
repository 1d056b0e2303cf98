"""Shared by tests/test_plain_key_gpu.py and tests/test_plain_key_emu.py: plain commitment keys (tuning msm_plain = 1 when the key is
created: the bases alone, every MSM through the plain flow) -- the key's bookkeeping and the scalars at the boundaries of the signed
16-bit digits and of the window weights 2^(16 w)."""
import numpy as np

TUNE = dict(msm_plain=1)          # read when the key is created; nothing is needed at a commit

# a digit: zero, +-1, the largest positive value below the tie, the tie 0x8000 (stays positive), the first value that borrows, a full
# window (0xFFFF -> -1 and a carry), and the carry's own window
DIGIT_VALUES = (0, 1, 2, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 0x10000, 0x10001)


def plain_key(S, cid, bases, **kw):
    """A plain key over `bases` with the bookkeeping every such key must show."""
    with S.tuning(**TUNE):
        ck = S.CommitmentKey(cid, bases, **kw)
    check_bookkeeping(ck, len(bases))
    return ck


def check_bookkeeping(ck, n):
    assert ck.is_plain() and not ck.is_compact() and not ck.has_wide_table()
    assert ck.table_bytes() == 64 * n, (ck.table_bytes(), n)


def limbs16(limbs):
    """the integer whose 16-bit limbs are `limbs`, least significant first"""
    return sum(int(v) << (16 * i) for i, v in enumerate(limbs))


def boundary_ints(q):
    """Canonical ints below q (both curves' orders lie between 2^253 and 2^254): every DIGIT_VALUES entry in windows 0, 7 and 14 and its
    negative; q - 1, (q +- 1) / 2, 2^253; the tie in every window below the top; a carry through every window below the top (top limb
    0x2FFF: below both moduli); 2^(16 w) for every window."""
    vals = []
    for x in DIGIT_VALUES:
        for w in (0, 7, 14):
            vals += [x << (16 * w), (q - (x << (16 * w))) % q]
    vals += [q - 1, (q - 1) // 2, (q + 1) // 2, 1 << 253]
    vals.append(limbs16([0x8000] * 15))
    vals.append(limbs16([0x8001] * 15 + [0x2FFF]))
    vals += window_powers()
    assert all(0 <= v < q for v in vals)
    return vals


def window_powers():
    return [1 << (16 * w) for w in range(16)]


def one_bucket_ints(q):
    """Scalars that, repeated, put every entry of a window into ONE bucket: zero (no entry at all), +-1, the tie, its neighbour (two
    windows), a high window alone."""
    return [0, 1, q - 1, 0x8000, 0x8001, 1 << 240]


def commit_counted(ck, v, **kw):
    """ck.commit(v), asserting that the key counted it as a set outside slot mode and nowhere else."""
    before = ck.msm_stats()
    got = ck.commit(v, **kw)
    after = ck.msm_stats()
    assert after["other_sets"] > before["other_sets"], (before, after)
    assert (after["slot_sets"], after["hot_sets"], after["redo"]) == (before["slot_sets"], before["hot_sets"], before["redo"]), (before, after)
    return got


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
