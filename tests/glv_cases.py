"""Shared by tests/test_glv_host.py (CPU) and tests/test_compact_key_gpu.py: the endomorphism split through the library's host entries
(srs_glv_constants / srs_glv_decompose: the body the digit kernel runs) and the scalars at which it is most likely to go wrong."""
import ctypes
import importlib.util
import os

import numpy as np

from conftest import ROOT

M64 = (1 << 64) - 1


def generator_module():
    spec = importlib.util.spec_from_file_location("gen_glv_consts", os.path.join(ROOT, "tools", "gen_glv_consts.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def limbs(vals):
    out = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, v in enumerate(vals):
        for j in range(4):
            out[i, j] = (v >> (64 * j)) & M64
    return out


def ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in a]


def constants(lib, cid):
    """(lambda, beta) of curve `cid` as python ints."""
    lam, beta = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    assert lib.srs_glv_constants(cid, lam.ctypes.data, beta.ctypes.data) == 0
    return ints(lam)[0], ints(beta)[0]


def decompose(lib, cid, scalars, repr_):
    """scalars: (n, 4) uint64 in form `repr_` -> list of signed (k1, k2)."""
    sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
    n = sc.shape[0]
    k1, k2 = np.zeros((n, 4), np.uint64), np.zeros((n, 4), np.uint64)
    n1, n2 = ctypes.c_int(), ctypes.c_int()
    p1, p2 = ctypes.byref(n1), ctypes.byref(n2)
    a, b, c = sc.ctypes.data, k1.ctypes.data, k2.ctypes.data
    fn = lib.srs_glv_decompose
    s1, s2 = [0] * n, [0] * n
    for i in range(n):
        assert fn(cid, a + 32 * i, repr_, b + 32 * i, c + 32 * i, p1, p2) == 0
        s1[i], s2[i] = n1.value, n2.value
    return [(-x if f else x, -y if g else y) for x, y, f, g in zip(ints(k1), ints(k2), s1, s2)]


def fixed_scalars(order, lam):
    return [0, 1, 2, order - 1, order - 2, lam, lam + 1, lam - 1, (1 << 128) - 1, 1 << 253, (order - 1) // 2]


def boundary_scalars(order, basis_entries, count, seed):
    """floor((2 j + 1) order / (2 |b|)) + {-1, 0, 1}: where a rounded quotient k |b| / order steps, for `count` seeded j per basis entry."""
    rng = np.random.default_rng(seed)
    out = []
    for b in basis_entries:
        b = abs(b)
        for _ in range(count):
            j = int.from_bytes(rng.bytes(16), "little") % b
            k = (2 * j + 1) * order // (2 * b)
            out += [x for x in (k - 1, k, k + 1) if 0 <= x < order]
    return out


def extreme_scalars(lib, cid, order, count=1000, seed=11):
    """The scalars with the largest |k1| and the largest |k2| among the rounding boundaries (canonical ints)."""
    g = generator_module()
    name, p, n, b, G = g.CURVES[cid]
    assert n == order
    c = g.derive(p, n, b, G)
    cand = boundary_scalars(order, (c["a1"], c["b1"], c["a2"], c["b2"]), count, seed)
    parts = decompose(lib, cid, limbs(cand), 1)
    i1 = max(range(len(cand)), key=lambda i: abs(parts[i][0]))
    i2 = max(range(len(cand)), key=lambda i: abs(parts[i][1]))
    return cand[i1], cand[i2]
