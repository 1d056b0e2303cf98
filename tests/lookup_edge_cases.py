"""Adversarial inputs for the lookup coefficients, shared by the GPU parity tests (tests/test_lookup_gpu.py) and their CPU twins on the
emulator (tests/test_emu_logic.py).  tests/lookup_cases.py feeds the multiplicity hash table small integers that are all present
in the table; here the table sees what it is built for and never met:

  collision_case     every key starts its probe chain in the LAST slot: chains as long as the table half, the wrap-around of the
                     probe step, looked-up values that are absent (the empty-slot exit of k_m_count), repeats of a table value in
                     another workgroup than its first occurrence (atomicMin onto a slot a different row claimed)
  limb_case          keys that differ in limb 7 only / in limb 0 only, looked-up words that match a table value in seven limbs
  contention_case    one value in every row (all rows on one atomicMin / atomicAdd), nothing found, a permutation at load factor 1/2
  hg_edge_case       l + r == 0 and t + r == 0 (1/0 := 0) at every position of one thread's chunk, in whole chunks, in the last element
  assigned_edge_case batch_invert_assigned with every denominator zero and a chunk of Zero / Trivial / Rational(n, 0) cells
  log_derivative_count_case   is_sat_log_derivative counts 0, 1 and 2 violated lookups

The lookup is a bare column pair (no selectors, one fixed column t, one advice column l, no gates), so ls[0] == l and ts[0] == t bit for
bit and arbitrary field elements reach the table.  Any 4 x u64 word below p is a valid Montgomery word and the kernels hash and compare
the words, so inputs are chosen as WORDS; the oracle sees mont_to_ints of them.  Expected values come from oracle/lookup.py and Python
ints only.  fe_hash / table_capacity restate the product's hash and capacity rule ONLY to choose inputs; tests/test_lookup_hash_pins.py
fails when csrc/rowprog.hip stops matching them.
"""
import functools

import numpy as np

from oracle import lookup as OL
from oracle import pyref as P

HASH_SEED, HASH_MUL, HASH_SHIFT = 0x9E3779B9, 0x85EBCA6B, 15
_M32 = np.uint64(0xFFFFFFFF)


def fe_hash(words):
    """(n, 4) uint64 words -> (n,) hash of the eight 32-bit limbs, as fe_hash of csrc/rowprog.hip."""
    limbs = np.ascontiguousarray(words, dtype=np.uint64).reshape(-1, 4).view(np.uint32).astype(np.uint64)      # little endian: (n, 8)
    h = np.full(limbs.shape[0], HASH_SEED, dtype=np.uint64)
    for i in range(8):
        h ^= limbs[:, i]
        h = (h * np.uint64(HASH_MUL)) & _M32
        h ^= h >> np.uint64(HASH_SHIFT)
    return h


def table_capacity(rows):
    """lookup_coeff_1: the smallest power of two >= 2 * rows, at least 2."""
    cap = 2
    while cap < 2 * rows:
        cap <<= 1
    return cap


def rand_words(rng, n):
    """n random words below p (either field): top word masked to 60 bits"""
    w = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    w[:, 3] &= np.uint64((1 << 60) - 1)
    return w


def _host(x):
    return x.cpu().numpy().view(np.uint64) if type(x).__module__.startswith("torch") else x


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


def _distinct(words):
    return len({w.tobytes() for w in words}) == len(words)


def column_pair_m(S, O, field, k, l, t, device=False):
    """m of the bare column-pair lookup l in t through lookup_coeff_1 (canonical ints), after asserting it against evaluate_m."""
    X = S.expression
    rows = 1 << k
    assert l.shape == t.shape == (rows, 4)
    St = S.PlonkStructure(field, k, [], [t], 1, [], lookups=[([X.Polynomial(1)], [X.Polynomial(0)])])
    try:
        ls, ts, ms = St.lookup_coeff_1(_dev(l) if device else l, np.zeros(4, np.uint64))
        assert np.array_equal(_host(ls[0]), l) and np.array_equal(_host(ts[0]), t)
        want = OL.evaluate_m(O.mont_to_ints(field, l), O.mont_to_ints(field, t))
        m = _host(ms[0])
        got = O.mont_to_ints(field, m)
        bad = [i for i in range(rows) if got[i] != want[i]]
        assert not bad, (len(bad), [(i, got[i], want[i]) for i in bad[:8]])
        assert np.array_equal(m, O.ints_to_mont(field, want))
        return got
    finally:
        St.close()


@functools.lru_cache(maxsize=None)
def last_slot_keys(k, seed=5):
    """rows + rows / 2 distinct words whose probe chain starts in the last slot of the 2^k-row table (searched once per size; callers only
    read the result)"""
    rows = 1 << k
    cap = table_capacity(rows)
    need = rows + rows // 2
    cand = rand_words(np.random.default_rng(seed), 2 * need * cap)
    keys = cand[(fe_hash(cand) & np.uint64(cap - 1)) == np.uint64(cap - 1)]
    assert keys.shape[0] >= need, (keys.shape[0], need)
    keys = keys[:need]
    assert _distinct(keys)
    return keys


def collision_case(S, O, field, k, device=False):
    rows = 1 << k
    keys = last_slot_keys(k)
    need = keys.shape[0]
    half = keys[: rows // 2]
    t = np.ascontiguousarray(np.concatenate([half, half[::-1]]))          # first occurrences below, the repeats mirrored above
    rng = np.random.default_rng(50 + k)
    l = np.ascontiguousarray(keys[rng.integers(0, need, size=rows)])      # keys[rows / 2:] are not in the table
    m = column_pair_m(S, O, field, k, l, t, device)
    assert 0 < sum(m) < rows
    assert not any(m[rows // 2:])


def limb_case(S, O, field, k=8):
    rows = 1 << k
    g = rows // 2
    rng = np.random.default_rng(8)
    base = rand_words(rng, 1)[0].view(np.uint32).copy()                   # eight limbs
    fresh = lambda hi, avoid: np.array([v for v in dict.fromkeys(rng.integers(0, hi, size=2 * rows).tolist()) if v != avoid], dtype=np.uint32)
    top = fresh(0x30000000, int(base[7]))                                 # limb 7 below p's 0x30644e72
    low = fresh(1 << 32, int(base[0]))
    assert len(top) >= g + 24 and len(low) >= g + 20

    def variants(limb, values):
        w = np.repeat(base[None, :], len(values), axis=0)
        w[:, limb] = values
        return w.view(np.uint64)
    t = np.ascontiguousarray(np.concatenate([variants(7, top[:g]), variants(0, low[:g])]))
    assert _distinct(t)
    # table values of both groups in turn, value number i looked up 1 + i % 3 times, on three quarters of the rows ...
    order = [j // 2 + (j % 2) * g for j in range(rows)]
    picks = [i for i in order for _ in range(1 + i % 3)][: rows - rows // 4]
    # ... and words that are NOT in the table and match table values in seven limbs: a fresh limb 7, a fresh limb 0, a changed limb 3
    mid = t[rng.integers(0, rows, size=rows // 4 - 44)].view(np.uint32).copy()
    mid[:, 3] ^= np.uint32(0x00010000)
    miss = np.concatenate([variants(7, top[g:g + 24]), variants(0, low[g:g + 20]), mid.view(np.uint64)])
    tset = {w.tobytes() for w in t}
    assert not any(w.tobytes() in tset for w in miss)
    l = np.concatenate([t[picks], miss])
    assert l.shape[0] == rows
    l = np.ascontiguousarray(l[rng.permutation(rows)])
    m = column_pair_m(S, O, field, k, l, t)
    assert sum(m) == len(picks) and max(m) == 3


def contention_case(S, O, field, k=10):
    rows = 1 << k
    rng = np.random.default_rng(10 + k)
    w = rand_words(rng, 2 * rows + 1)
    assert _distinct(w)
    same = np.ascontiguousarray(np.repeat(w[:1], rows, axis=0))
    m = column_pair_m(S, O, field, k, same, same)                         # (a) every row on one slot
    assert m[0] == rows and not any(m[1:])
    m = column_pair_m(S, O, field, k, np.ascontiguousarray(w[1:rows + 1]), same)         # (b) nothing found
    assert not any(m)
    t = np.ascontiguousarray(w[rows + 1:])
    m = column_pair_m(S, O, field, k, np.ascontiguousarray(t[rng.permutation(rows)]), t)  # (c) a permutation, load factor 1/2
    assert all(v == 1 for v in m)


HG_SIZES = (1, 127, 129, 1023, 1025, 2049)


def hg_challenges(field):
    return (0, 1, P.MODULI[field] - 1, 0x1234567)


@functools.lru_cache(maxsize=None)
def _hg_inputs(field, n, r):
    """-> l, t, m, expected h, expected g (canonical ints) and the positions where l + r == 0; computed once per (field, n, r)"""
    p = P.MODULI[field]
    rng = np.random.default_rng(1000 * n + r % 1000)
    rnd = lambda: [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) for _ in range(n)]
    l, t = rnd(), rnd()
    m = [int(v) for v in rng.integers(0, 5, size=n)]
    neg_r = (p - r) % p
    zeros_l = set(range(0, n, 128)) | {n - 1}
    if n >= 1024:
        zeros_l |= {5 + 128 * j for j in range(8)}                        # one whole chunk: its running product stays one
    for i in zeros_l:
        l[i] = neg_r
    for i in range(3, n, 5):
        t[i], m[i] = neg_r, 3
    want_h, want_g = OL.evaluate_h_g(l, t, r, m, p)                       # inv(0) = 0 there
    assert all(want_h[i] == 0 for i in zeros_l) and all(want_g[i] == 0 for i in range(3, n, 5))
    assert sum(1 for v in want_h if v == 0) == len(zeros_l) and sum(1 for v, c in zip(want_g, m) if v == 0 and c) == len(range(3, n, 5))
    return l, t, m, want_h, want_g, sorted(zeros_l)


def hg_edge_case(S, O, field, n, r, device=False):
    """evaluate_h_g through lookup_coeff_2 (no structure needed) with l + r == 0 / t + r == 0 planted; k_lookup_hg gives thread x of
    block 0 the elements x + 128 j, j < 8."""
    l, t, m, want_h, want_g, zeros_l = _hg_inputs(field, n, r)
    St = type("LookupOnly", (), {"field": field, "lookup_coeff_2": S.PlonkStructure.lookup_coeff_2})()
    put = _dev if device else (lambda x: x)
    lw, tw, mw = (O.ints_to_mont(field, v) for v in (l, t, m))
    hs, gs = St.lookup_coeff_2([put(lw)], [put(tw)], [put(mw)], O.ints_to_mont(field, [r])[0])
    h, g = _host(hs[0]), _host(gs[0])
    assert O.mont_to_ints(field, h) == want_h, (field, n, r)
    assert O.mont_to_ints(field, g) == want_g, (field, n, r)
    assert not h[zeros_l].any() and not g[3::5].any()                     # 1/0 is the all-zero word


def assigned_edge_case(S, O, field):
    p = P.MODULI[field]
    rng = np.random.default_rng(60 + field)
    rnd = lambda n: [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % p for _ in range(n)]
    for n in (8, 1024, 1025):                                             # every denominator zero
        num = rnd(n)
        has = rng.integers(0, 2, size=n).astype(np.uint8)
        has[0], has[n - 1] = 1, 0
        numw, zero = O.ints_to_mont(field, num), np.zeros((n, 4), np.uint64)
        got = S.batch_invert_assigned(field, numw, zero, has)
        assert O.mont_to_ints(field, got) == [0 if f else a for a, f in zip(num, has)], n
        assert not S.batch_invert_assigned(field, numw, zero).any(), n
    # one thread's chunk (elements 6 + 128 j) holds Zero / Trivial / Rational(n, 0) cells only; everything around it is Rational
    n = 1031
    num, den = rnd(n), rnd(n)
    has = np.ones(n, np.uint8)
    for j in range(8):
        i = 6 + 128 * j
        if j % 3 == 0:
            num[i], has[i] = 0, 0                                         # Assigned::Zero
        elif j % 3 == 1:
            has[i] = 0                                                    # Assigned::Trivial
        else:
            den[i] = 0                                                    # Assigned::Rational(n, 0)
    inv = lambda x: pow(x, p - 2, p) if x else 0
    numw, denw = O.ints_to_mont(field, num), O.ints_to_mont(field, den)
    assert O.mont_to_ints(field, S.batch_invert_assigned(field, numw, denw, has)) == [a * inv(d) % p if f else a for a, d, f in zip(num, den, has)]
    assert O.mont_to_ints(field, S.batch_invert_assigned(field, numw, denw)) == [a * inv(d) % p for a, d in zip(num, den)]


def _violated_lookups(O, field, W_last, num_lookups, rows, p):
    """PlonkStructure::is_sat_log_derivative (src/plonk/mod.rs:366-398), counting instead of `all`: the lookups i whose
    sum_row (h_i - g_i) != 0, h_i / g_i = vectors 2 i / 2 i + 1 of the last round."""
    vals = O.mont_to_ints(field, W_last)
    vec = lambda idx: vals[idx * rows:(idx + 1) * rows]
    return sum(1 for i in range(num_lookups) if sum(a - b for a, b in zip(vec(2 * i), vec(2 * i + 1))) % p != 0)


def log_derivative_count_case(S, O, field):
    from lookup_cases import _circuit, _shape, _to_product_expr
    X = S.expression
    p = P.MODULI[field]
    for variant, k in (("two", 6), ("scalar", 10)):
        rows = 1 << k
        rng = np.random.default_rng(70 + k)
        ns, nf, na, ogates, olookups = _shape(variant)
        selectors, fixed, _ = _circuit(O, field, variant, k, rng)
        meta = OL.build_metainfo(k, ns, nf, na, ogates, olookups)
        St = S.PlonkStructure(field, k, selectors, fixed, na, [_to_product_expr(X, g) for g in ogates],
                              lookups=[([_to_product_expr(X, e) for e in i], [_to_product_expr(X, e) for e in t]) for i, t in olookups])
        nl = St.num_lookups
        assert nl == meta.num_lookups == (2 if variant == "two" else 1) and not St.has_vector_lookup
        hg = []
        for _ in range(nl):                                               # g_i a permutation of h_i: the sums agree
            h = rand_words(rng, rows)
            hg += [h, h[rng.permutation(rows)]]
        W0 = rand_words(rng, (na + 3 * nl) * rows)
        other = rand_words(rng, 1)[0]

        def check(want):
            W = [W0, np.ascontiguousarray(np.concatenate(hg))]
            assert _violated_lookups(O, field, W[1], nl, rows, p) == want
            assert OL.is_sat_log_derivative(O, field, meta, W, rows, p) == (want == 0)
            assert St.is_sat_log_derivative(W) == want, (variant, want)
        check(0)
        g_last = hg[2 * nl - 1] = hg[2 * nl - 1].copy()
        g_last[rows - 1 if k == 10 else 17] = other                       # the last lookup's g; at k = 10 in the last row
        check(1)
        if nl == 2:
            hg[1] = hg[1].copy()
            hg[1][40] = other                                             # g_0 as well
            check(2)
        St.close()
