"""CPU: the cases of tests/space_cases.py on the emulator build (tests/emu/libsirius_emu.so compiles the same csrc/capi.hip): host
operands go through the staging, device operands are NumPy memory passed as SRS_SPACE_DEVICE.

An emulated MSM takes ~2.5 s whatever its length, so of the commits this twin keeps the two staging forms only -- one batch of unequal
lengths (host scalars staged) and the commitments-only cross terms (T vectors as temporaries in either space); the commits at every
size and the key's arena growing between them run in the GPU twin."""
import os
import subprocess

import pytest

import space_cases as SC
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
    k = SC.make_key(emu, oracle)
    yield k
    k[0].close()


@pytest.mark.parametrize("n", SC.VECTOR_SIZES)
def test_emu_vector_entries(emu, oracle, sp, key, n):
    for field in (0, 1):
        for n_terms in (0, 1, 3):
            SC.fold_case(emu, oracle, sp, field, n, n_terms)
        SC.lookup_hg_case(emu, oracle, sp, field, n)
        SC.assigned_case(emu, oracle, sp, field, n)
    for J in (1, 3):
        SC.lincomb_case(emu, oracle, sp, n, J)
    if n == 9:
        SC.commit_batch_case(emu, oracle, sp, key, n)
    SC.sparse_case(emu, oracle, sp, n)


@pytest.mark.parametrize("shape", SC.NTT_SHAPES)
def test_emu_ntt_batch(emu, oracle, sp, shape):
    SC.ntt_case(emu, oracle, sp, *shape)


@pytest.mark.parametrize("k", SC.STRUCTURE_KS)
def test_emu_main_gate_structure(emu, oracle, sp, key, k):
    SC.main_gate_case(emu, oracle, sp, k, key if k == 4 else None, commit_forms=(False,))


@pytest.mark.parametrize("k", SC.STRUCTURE_KS)
def test_emu_lookup_structure(emu, oracle, sp, k):
    SC.lookup_structure_case(emu, oracle, sp, k)


def test_emu_arenas_regrow(emu, oracle, sp):
    SC.regrow_case(emu, oracle, sp)
