"""CPU: plain commitment keys of form 2 (tuning msm_plain = 2: the bases alone, 8 windows per MSM through the endomorphism) on the emulator
build of the product kernels -- the split digits, the grouping of two entries per scalar into 8 windows, the flagged entries of level 0
over the one table, the 8 linked bucket sets beside 8 empty segments and the Horner chain of 8 window weights, against the oracle.  Every
case runs in a process of its own with the emulator library loaded (as test_plain_key_emu does), so this file launches no emulated kernel
in the pytest process.  An emulated flow of this kind costs seconds whatever its size: few commits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seeded_scalars

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libsirius_emu.so")


@pytest.fixture(scope="module")
def emu_built():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j4"], stdout=subprocess.DEVNULL)


def _in_emulator(case, *args):
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            f"from sirius_amd import _lib; _lib.load({EMU_LIB!r})\n"
            "import oracle, sirius_amd, test_plain_glv_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid", [0, 1])
def test_emu_plain_glv_commit(emu_built, cid):
    _in_emulator("_commit_case", cid)


def test_emu_plain_glv_streamed_and_batch(emu_built):
    _in_emulator("_streamed_and_batch_case")


def _commit_case(emu, oracle, cid):
    from oracle import pyref as P
    from sirius_amd import _lib
    from plain_glv_cases import KEY_N, boundary_vector, boundary_vector_ints, commit_counted, glv_plain_key, split_coverage
    O = oracle
    q = P.CURVES[cid].q
    bases = O.make_bases(cid, 51 + cid, KEY_N)
    ck = glv_plain_key(emu, cid, bases)
    signs, k1_zero, k2_zero = split_coverage(_lib.lib(), cid, boundary_vector_ints(_lib.lib(), cid, q))
    assert len(signs) == 4 and k1_zero and k2_zero                      # a condition on the inputs
    edge = boundary_vector(O, _lib.lib(), cid, q, KEY_N, 4)
    for sc in (edge, seeded_scalars(O, cid, KEY_N, 5, "trace"), seeded_scalars(O, cid, 1, 6, "uniform")):
        assert np.array_equal(commit_counted(ck, sc), O.msm(cid, sc, bases[:len(sc)])), len(sc)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    ck.close()


def _streamed_and_batch_case(emu, oracle):
    from plain_glv_cases import KEY_N, TUNE, check_form2, glv_plain_key
    O = oracle
    cid = 1
    bases = O.make_bases(cid, 57, KEY_N)
    ck = glv_plain_key(emu, cid, bases)
    sc = seeded_scalars(O, cid, KEY_N, 7, "trace")
    before = ck.msm_stats()
    with emu.tuning(commit_chunks=3):
        assert np.array_equal(ck.commit_upload(sc), O.msm(cid, sc, bases))
    after = ck.msm_stats()
    assert after["other_sets"] > before["other_sets"] and after["slot_sets"] == before["slot_sets"], (before, after)
    vs = [seeded_scalars(O, cid, n, 8 + n, "uniform") for n in (300, 63, 1)]
    assert np.array_equal(ck.commit_batch(vs), np.stack([O.msm(cid, v, bases[:len(v)]) for v in vs]))
    ck.close()
    with emu.tuning(**TUNE):
        empty = emu.CommitmentKey(cid, bases[:0])
    check_form2(empty, 0)
    empty.close()
