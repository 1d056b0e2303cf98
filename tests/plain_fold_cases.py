"""Shared by tests/test_plain_fold_gpu.py and tests/test_plain_fold_emu.py: streamed commits on plain commitment keys (tuning msm_plain = 1
or 2) whose chunks fold their finished window buckets into the key's running buckets, one set per window -- the streamed commit counted
through plain_stats(), the scalars and the bases at which the fold can go wrong.  Every result is compared with the oracle's MSM."""
import numpy as np

import glv_cases as G
import plain_glv_cases as F2
import plain_key_cases as F1

CHUNKS = 3                        # tuning commit_chunks: equal chunks cut at multiples of 1024 scalars
N_FULL = 3072                     # 1024 / 1024 / 1024
N_RAGGED = 2053                   # 1024 / 1024 / 5: the last set has few entries, every bucket of it is single
DIGITS = (1, 0x7FFF, 0x8000)      # a digit of the degenerate-base cases: the smallest, the largest below the tie, the tie


def order(cid):
    from oracle import pyref as P
    return P.CURVES[cid].q


def fold_key(S, cid, form, bases):
    """A plain key of `form` over `bases` with the bookkeeping every such key must show."""
    return F1.plain_key(S, cid, bases) if form == 1 else F2.glv_plain_key(S, cid, bases)


def counted(ck, run, fold_sets, reductions):
    """run(), asserting what the key counted meanwhile: sets folded into the running buckets and bucket reductions of the plain flow --
    and that no set went anywhere but the plain flow.  A condition on the inputs of a test, not the thing under test."""
    before, mb = ck.plain_stats(), ck.msm_stats()
    got = run()
    after, ma = ck.plain_stats(), ck.msm_stats()
    assert (after["fold_sets"] - before["fold_sets"], after["reductions"] - before["reductions"]) == (fold_sets, reductions), (before, after)
    assert (ma["slot_sets"], ma["hot_sets"], ma["redo"]) == (mb["slot_sets"], mb["hot_sets"], mb["redo"]) == (0, 0, 0), (mb, ma)
    return got


def streamed(S, ck, v, sets=CHUNKS, **kw):
    """ck.commit_upload(v) in CHUNKS chunks, asserting that it folded `sets` sets under one reduction."""
    with S.tuning(commit_chunks=CHUNKS):
        return counted(ck, lambda: ck.commit_upload(v, **kw), sets, 1)


def boundary_scalars(O, lib, cid, form, n, seed):
    """(n, 4) Montgomery scalars: the form's boundary vector (digit, window-weight and, form 2, split boundaries) in the first chunk,
    uniform fill, and five boundary values at the very end -- the whole of the last chunk of N_RAGGED."""
    from conftest import seeded_scalars
    q = order(cid)
    vals = F1.boundary_ints(q) if form == 1 else F2.boundary_vector_ints(lib, cid, q)
    assert len(vals) < 1024
    tail = [q - 1, 0x8000, F1.limbs16([0x8001] * 15 + [0x2FFF]), 1 << 240, (q + 1) // 2]
    sf = O.SCALAR_FIELD[cid]
    fill = seeded_scalars(O, cid, n - len(vals) - len(tail), seed, "uniform")
    return np.concatenate([O.ints_to_mont(sf, vals), fill, O.ints_to_mont(sf, tail)])


def one_bucket_values(lib, cid, form):
    q = order(cid)
    return F1.one_bucket_ints(q) if form == 1 else F2.one_bucket_ints(G.constants(lib, cid)[0], q)


def zero_chunk(v, j):
    """`v` with the whole of chunk j (of N_FULL scalars in CHUNKS chunks) set to zero"""
    out = v.copy()
    out[1024 * j:1024 * (j + 1)] = 0
    return out


def degenerate_bases(O, lib, cid, form, seed, n=N_FULL):
    """Oracle bases with bases[1024] = bases[0] and bases[2048] = -bases[0]: the same point, and its opposite, in different chunks.
    Form 2 also has bases[1025] = phi(bases[0]) = (beta x, y)."""
    bf = O.BASE_FIELD[cid]
    bases = O.make_bases(cid, seed, n)
    P0 = bases[0].copy()
    neg = P0.copy()
    neg[4:] = O.fe_sub(bf, np.zeros((1, 4), np.uint64), P0[None, 4:])[0]
    bases[1024], bases[2048] = P0, neg
    if form == 2:
        lam, beta = G.constants(lib, cid)
        phi = P0.copy()
        phi[:4] = O.fe_mul(bf, P0[None, :4], O.ints_to_mont(bf, [beta]))[0]
        bases[1025] = phi
        assert np.array_equal(O.msm(cid, O.ints_to_mont(O.SCALAR_FIELD[cid], [lam]), bases[:1]), phi)       # beta matches lambda
    assert all(O.is_on_curve(cid, bases[i]) for i in (0, 1024, 1025, 2048))
    return bases


def degenerate_heads(lib, cid, form, d):
    """name -> {index: canonical scalar}: what meets in a running bucket.  "double": P of chunk 0 and P of chunk 1 (the fold's addition is
    a doubling); "cancel": P of chunk 0 and -P of chunk 2 (the bucket returns to the identity); "endo" (form 2): a flagged entry of P in
    chunk 0 and the unflagged phi(P) of chunk 1 (the same point again)."""
    q = order(cid)
    heads = {"double": {0: d, 1024: d}, "cancel": {0: d, 2048: d}}
    if form == 2:
        lam, _ = G.constants(lib, cid)
        heads["endo"] = {0: lam * d % q, 1025: d}
    return heads


def with_head(O, cid, head, fill, n=N_FULL):
    """(n, 4) Montgomery scalars: `head` at its indices, `fill` (canonical ints, or None for zeros) elsewhere"""
    vals = [0] * n if fill is None else list(fill[:n])
    for i, x in head.items():
        vals[i] = x
    return O.ints_to_mont(O.SCALAR_FIELD[cid], vals)
