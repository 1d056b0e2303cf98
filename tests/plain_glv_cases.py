"""Shared by tests/test_plain_glv_gpu.py and tests/test_plain_glv_emu.py: plain commitment keys of form 2 (tuning msm_plain = 2 when the
key is created: the bases alone, every MSM over the split scalar k = k1 + lambda k2 in 8 windows) -- the key's bookkeeping and the vector of
scalars at the boundaries of the signed 16-bit digits, of the window weights and of the split.  Every result is compared with the oracle."""
import numpy as np

import glv_cases as G
from plain_key_cases import boundary_ints, check_bookkeeping, commit_counted, dev  # noqa: F401  (re-exported to the two test files)

TUNE = dict(msm_plain=2)          # read when the key is created; nothing is needed at a commit
KEY_N = 1100                      # two tile boundaries of the segment passes (WIDE_TILE = 512) and a last tile of 76 scalars


def glv_plain_key(S, cid, bases, **kw):
    """A plain key of form 2 over `bases` with the bookkeeping every such key must show."""
    with S.tuning(**TUNE):
        ck = S.CommitmentKey(cid, bases, **kw)
    check_form2(ck, len(bases))
    return ck


def check_form2(ck, n):
    assert ck.plain_form() == 2, ck.plain_form()
    check_bookkeeping(ck, n)          # is_plain(), not compact, no wide table, table_bytes() == 64 n


def basis(cid, order):
    """The four entries of the reduced lattice basis the split rounds against (tools/gen_glv_consts.py)."""
    g = G.generator_module()
    _, p, n, b, gen = g.CURVES[cid]
    assert n == order
    c = g.derive(p, n, b, gen)
    return c["a1"], c["b1"], c["a2"], c["b2"]


def boundary_vector_ints(lib, cid, q):
    """Canonical ints: the digit and window boundaries of a plain key (boundary_ints), the fixed scalars of the split (0, +-1, lambda with
    k1 = 0, lambda +- 1, 2^128 - 1, ...), 36 scalars around the points where a rounded quotient of the split steps, and the two scalars with
    the largest |k1| and |k2| (the top window of a half)."""
    lam, _ = G.constants(lib, cid)
    vals = boundary_ints(q) + G.fixed_scalars(q, lam) + G.boundary_scalars(q, basis(cid, q), 3, 17 + cid)
    vals += list(G.extreme_scalars(lib, cid, q))
    assert all(0 <= v < q for v in vals)
    return vals


def split_coverage(lib, cid, vals):
    """What the split makes of `vals` (the body the digit kernel runs): the set of sign pairs (k1 < 0, k2 < 0) among the scalars with both
    halves non-zero, whether a scalar has k1 = 0 (and k2 != 0), and whether one has k2 = 0 (and k1 != 0)."""
    parts = G.decompose(lib, cid, G.limbs(vals), 1)
    signs = {(a < 0, b < 0) for a, b in parts if a and b}
    return signs, any(a == 0 and b != 0 for a, b in parts), any(b == 0 and a != 0 for a, b in parts)


def boundary_vector(O, lib, cid, q, n, seed):
    """(n, 4) Montgomery scalars: the first min(n, len) entries of boundary_vector_ints, then uniform fill."""
    from conftest import seeded_scalars
    vals = boundary_vector_ints(lib, cid, q)[:n]
    head = O.ints_to_mont(O.SCALAR_FIELD[cid], vals)
    if n == len(vals):
        return head
    return np.concatenate([head, seeded_scalars(O, cid, n - len(vals), seed, "uniform")])


def one_bucket_ints(lam, q):
    """Scalars that, repeated, put every entry of a window into ONE bucket: zero (no entry), +-1 (k2 = 0), the tie of the lowest window,
    +-lambda (k1 = 0: flagged entries alone), lambda + 1 and the tie in both halves (a flagged and an unflagged entry per scalar in one
    bucket), and lambda 2^112 (the top window of k2)."""
    return [0, 1, q - 1, 0x8000, lam, q - lam, lam + 1, 0x8000 * (1 + lam) % q, (lam << 112) % q]
