"""CPU: the closed-form ProtoGalaxy sums of the reference's leaf rows.  The host helper against the naive sum over every
leaf in Python integers, and the cases of tests/test_pg_closed_form_gpu.py at k <= 8 (plus one k = 10) on the emulator library."""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libsirius_emu.so")


@pytest.fixture(scope="module")
def emu():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j4"], stdout=subprocess.DEVNULL)
    import sirius_amd as S
    from sirius_amd import _lib
    _lib.load(EMU_LIB)
    yield S
    _lib._lib = None          # the real library is (re)loaded lazily by later tests


def test_closed_form_helper_vs_naive_sum(oracle):
    """srs_pg_closed_form (host code) == sum_i pow_i(w) f_i over every leaf, f_i = c[i >> k] below n_gates 2^k and zero in the padding:
    the value for plain weights (evaluate_e, G at a point), and F's coefficients evaluated at random X for w_b = beta_b + X delta^(2^b)."""
    from oracle import pyref as P
    from sirius_amd import _lib
    O, FR = oracle, P.FR
    lib = _lib.load()
    rnd = random.Random(20)
    m = lambda v: O.ints_to_mont(O.FR, list(v))

    def pow_i(i, w):
        out = 1
        for b, wb in enumerate(w):
            if (i >> b) & 1:
                out = out * wb % FR
        return out

    for k in range(0, 7):
        for n_gates in range(1, 6):
            t = k + (n_gates - 1).bit_length()
            for extra in (0, 1):                      # more weights than k + log2(gates): a larger table, padded with zero leaves
                nw = t + extra
                c = [rnd.randrange(FR) for _ in range(n_gates)]
                w = [rnd.randrange(FR) for _ in range(nw)]
                delta = rnd.randrange(FR)
                leaf = lambda i: c[i >> k] if (i >> k) < n_gates else 0
                out = np.zeros((nw + 1, 4), np.uint64)
                cm, wm, dm = m(c), (m(w) if nw else np.zeros((1, 4), np.uint64)), m([delta])
                assert lib.srs_pg_closed_form(cm.ctypes.data, n_gates, k, wm.ctypes.data, nw, None, out.ctypes.data) == 0
                assert O.mont_to_ints(O.FR, out[:1]) == [sum(pow_i(i, w) * leaf(i) for i in range(1 << nw)) % FR], (k, n_gates, nw)
                assert lib.srs_pg_closed_form(cm.ctypes.data, n_gates, k, wm.ctypes.data, nw, dm.ctypes.data, out.ctypes.data) == 0
                coef = O.mont_to_ints(O.FR, out)
                deltas = [pow(delta, 1 << b, FR) for b in range(nw)]
                for X in (0, 1, rnd.randrange(FR)):
                    wx = [(b + X * d) % FR for b, d in zip(w, deltas)]
                    direct = sum(pow_i(i, wx) * leaf(i) for i in range(1 << nw)) % FR
                    assert sum(cf * pow(X, j, FR) for j, cf in enumerate(coef)) % FR == direct, (k, n_gates, nw, X)
    bad = np.zeros((4, 4), np.uint64)
    assert lib.srs_pg_closed_form(bad.ctypes.data, 3, 2, bad.ctypes.data, 3, None, bad.ctypes.data) == _lib.ERR_INVALID      # 3 gates need 2 bits


@pytest.mark.parametrize("k", [3, 7, 8])
@pytest.mark.parametrize("n_gates", [1, 2, 3])
def test_emu_closed_form_one_incoming_trace(emu, oracle, k, n_gates):
    from pg_closed_cases import run_closed_case
    run_closed_case(emu, oracle, k, n_gates, 1)


def test_emu_closed_form_k10_specialised_gate_set(emu, oracle):
    from pg_closed_cases import run_closed_case
    run_closed_case(emu, oracle, 10, ("main", [5, 3]), 1)


def test_emu_closed_form_three_incoming_traces(emu, oracle):
    """L = 3: G on the roots of unity, the inverse DFT on the host (a degree-2 gate keeps K at 256 points: the 2^16-point K of the GPU
    test's shape is unchanged code behind G)"""
    from pg_closed_cases import run_closed_case
    ctx = run_closed_case(emu, oracle, 4, "deg2", 3)
    assert (ctx.fft_points_count_G, ctx.fft_log_domain_size_K) == (8, 8)


@pytest.mark.parametrize("k,L", [(7, 1), (5, 3)])
def test_emu_closed_form_challenges_folded_per_point(emu, oracle, k, L):
    from pg_closed_cases import run_closed_case
    run_closed_case(emu, oracle, k, "primary+challenge", L)


@pytest.mark.parametrize("world", [2, 3])
def test_emu_closed_form_sharded_partials(emu, oracle, world):
    from pg_closed_cases import run_sharded_case
    run_sharded_case(emu, oracle, 8, 3, world)
