"""CPU: the cases of tests/test_pg_routes_gpu.py on the emulator library."""
import os
import subprocess

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


@pytest.mark.parametrize("k,gate_T", [(10, [5, 3]), (10, [2]), (11, [5, 3])])
def test_emu_reference_rows_every_route_same_bits(emu, oracle, k, gate_T):
    from pg_route_cases import run_reference_rows_case
    run_reference_rows_case(emu, oracle, k, gate_T)


_whole = {}      # (k, gates) -> the unsharded F, G, e of this module's library


@pytest.mark.parametrize("k,world,gate_T,nonzero_ranks", [(7, 2, [2], 1), (11, 2, [5, 3], 2), (11, 3, [5, 3], 2), (11, 3, [2], 2)])
def test_emu_true_rows_sharded_partials(emu, oracle, k, world, gate_T, nonzero_ranks):
    from pg_route_cases import run_sharded_true_rows_case
    run_sharded_true_rows_case(emu, oracle, k, world, gate_T, nonzero_ranks, _whole)
