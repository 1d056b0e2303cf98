"""CPU, no device: the endomorphism split behind compact commitment keys.  The generated constants are current, lambda / beta are
matching cube roots of unity (checked on oracle points), and srs_glv_decompose -- the body k_digits runs for a compact key --
satisfies k1 + lambda k2 = k with |k1|, |k2| < 2^127 at the fixed scalars, at the rounding boundaries and on 100 000 uniform scalars
per curve in both input forms."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import glv_cases as G


@pytest.fixture(scope="module")
def lib():
    from sirius_amd import _lib
    return _lib.load()


def _order(cid):
    from oracle import pyref as P
    return P.CURVES[cid].q


def test_generated_glv_consts_are_current(tmp_path):
    out = tmp_path / "glv_consts.inc"
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "gen_glv_consts.py"), str(out)], stdout=subprocess.DEVNULL)
    assert out.read_text() == open(os.path.join(ROOT, "sirius_amd", "csrc", "glv_consts.inc")).read(), \
        "glv_consts.inc is not what tools/gen_glv_consts.py generates"


@pytest.mark.parametrize("cid", [0, 1])
def test_glv_constants(lib, oracle, cid):
    O = oracle
    from oracle import pyref as P
    n, p = _order(cid), P.MODULI[O.BASE_FIELD[cid]]
    assert n == P.MODULI[O.SCALAR_FIELD[cid]]
    lam, beta = G.constants(lib, cid)
    assert 1 < lam < n and pow(lam, 3, n) == 1
    assert 1 < beta < p and pow(beta, 3, p) == 1
    lam_m = O.ints_to_mont(O.SCALAR_FIELD[cid], [lam])[0]
    beta_m = O.ints_to_mont(O.BASE_FIELD[cid], [beta])[0]
    for pt in O.make_bases(cid, 31 + cid, 4):
        want = pt.copy()
        want[:4] = O.fe_mul(O.BASE_FIELD[cid], pt[:4], beta_m).reshape(4)
        assert np.array_equal(O.point_mul(cid, lam_m, pt), want)


def _check(cid, lam, scalars, parts):
    n = _order(cid)
    assert len(scalars) == len(parts)
    for k, (k1, k2) in zip(scalars, parts):
        assert (k1 + lam * k2 - k) % n == 0, hex(k)
        assert abs(k1) < 1 << 127 and abs(k2) < 1 << 127, hex(k)


@pytest.mark.parametrize("cid", [0, 1])
def test_glv_decompose_fixed_and_boundary_scalars(lib, oracle, cid):
    n = _order(cid)
    lam, _ = G.constants(lib, cid)
    g = G.generator_module()
    _, p, order, b, gen = g.CURVES[cid]
    c = g.derive(p, order, b, gen)
    assert order == n and c["lam"] == lam
    ks = G.fixed_scalars(n, lam) + G.boundary_scalars(n, (c["a1"], c["b1"], c["a2"], c["b2"]), 1000, 7)
    parts = G.decompose(lib, cid, G.limbs(ks), 1)
    _check(cid, lam, ks, parts)
    # the generator's integer model of the scheme is what the library computes, and its proven bound holds
    assert parts == [g.decompose(c, k) for k in ks]
    assert max(abs(a) for a, _ in parts) <= c["k1_max"] and max(abs(b_) for _, b_ in parts) <= c["k2_max"]
    mont = oracle.ints_to_mont(oracle.SCALAR_FIELD[cid], ks)
    assert G.decompose(lib, cid, mont, 0) == parts


@pytest.mark.parametrize("cid", [0, 1])
def test_glv_decompose_uniform_scalars(lib, oracle, cid):
    O = oracle
    n = _order(cid)
    lam, _ = G.constants(lib, cid)
    rng = np.random.default_rng(100 + cid)
    ks = [int.from_bytes(rng.bytes(40), "little") % n for _ in range(100_000)]
    canon = G.limbs(ks)
    parts = G.decompose(lib, cid, canon, 1)
    _check(cid, lam, ks, parts)
    assert G.decompose(lib, cid, O.to_mont(O.SCALAR_FIELD[cid], canon), 0) == parts
