"""CPU: srs_run_sps_protocol on the emulator build (tests/emu/libsirius_emu.so compiles the same csrc/capi.hip and csrc/rowprog.hip):
the cases of tests/sps_cases.py at the reference's sizes -- the three-round vector lookup at k = 5, the two-round scalar lookup at
k = 6 (and at k = 10 with the advice streamed in three chunks and the lookup coefficients as a further set of the same commit), the
one-challenge protocol without lookups at k = 5 -- and every refusal.  The device vector is NumPy memory passed as
SRS_SPACE_DEVICE.  An emulated MSM takes ~2.5 s whatever its length, so the commitment re-check (one more batched MSM per case) and
the larger sizes stay with the GPU twin."""
import os
import subprocess

import pytest

import space_cases as SC
import sps_cases as SPS
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


@pytest.fixture
def sp(monkeypatch):
    return SC.Spaces.emulator(monkeypatch)


@pytest.fixture(scope="module")
def key(emu, oracle):
    bases = oracle.make_bases(0, 11, 1 << 10)
    ck = emu.CommitmentKey(0, bases)
    yield ck, bases
    ck.close()


def test_emu_sps_vector_lookup(emu, oracle, sp, key):
    SPS.run_case(emu, oracle, sp, key, 0, "vector", 5, witness_commit=False)


def test_emu_sps_scalar_lookup(emu, oracle, sp, key):
    SPS.run_case(emu, oracle, sp, key, 0, "scalar", 6, witness_commit=False)


def test_emu_sps_scalar_lookup_chunked_advice(emu, oracle, sp, key):
    """round 0 of the two-round protocol with the advice in three streamed chunks (one per column) and (ls, ts, ms) as a fourth set of
    the same commit"""
    bases = oracle.make_bases(0, 11, 6 << 10)
    ck = emu.CommitmentKey(0, bases)
    with emu.tuning(commit_chunks=3):
        SPS.run_case(emu, oracle, sp, (ck, bases), 0, "scalar", 10, witness_commit=False, stepwise=False)
    ck.close()


def test_emu_sps_gates_without_lookups(emu, oracle, sp, key):
    SPS.run_case(emu, oracle, sp, key, 0, "gates", 5, space="dev", lens=[32, 29, 0], witness_commit=False)


def test_emu_sps_refusals(emu, oracle, sp, key):
    SPS.refusal_cases(emu, oracle, sp, key)
