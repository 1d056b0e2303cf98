"""CPU: compact commitment keys that also carry the 7-window wide table (tuning msm_compact = 2) on the emulator build of the product
kernels -- the split 20-bit digits of the segment passes, the flagged payloads over the second table and the beta product in level 0 of the
wide flow, against the oracle.  Every case runs in a process of its own with the emulator library loaded (as test_compact_key_emu does),
so this file launches no emulated kernel in the pytest process.  An emulated wide MSM costs seconds whatever its size: few commits."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, seeded_scalars

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libsirius_emu.so")
KEY_N = 1100


@pytest.fixture(scope="module")
def emu_built():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j4"], stdout=subprocess.DEVNULL)


def _in_emulator(case, *args):
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            f"from sirius_amd import _lib; _lib.load({EMU_LIB!r})\n"
            "import oracle, sirius_amd, test_compact_wide_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid", [0, 1])
def test_emu_compact_wide_commit(emu_built, cid):
    _in_emulator("_commit_case", cid)


def test_emu_compact_wide_fall_through(emu_built):
    _in_emulator("_fall_through_case")


def _commit_case(emu, oracle, cid):
    from oracle import pyref as P
    from sirius_amd import _lib
    from compact_wide_cases import TUNE, boundary_ints, commit_counted, compact_wide_key
    O = oracle
    bases = O.make_bases(cid, 27 + cid, KEY_N)
    ck = compact_wide_key(emu, cid, bases)
    vals = boundary_ints(_lib.lib(), cid, P.CURVES[cid].q)
    edge = np.concatenate([O.ints_to_mont(O.SCALAR_FIELD[cid], vals), seeded_scalars(O, cid, KEY_N - len(vals), 4, "uniform")])
    with emu.tuning(**TUNE):
        for sc in (edge, seeded_scalars(O, cid, KEY_N, 5, "trace"), seeded_scalars(O, cid, 1, 6, "uniform")):
            assert np.array_equal(commit_counted(ck, sc), O.msm(cid, sc, bases[:len(sc)])), len(sc)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    ck.close()


def _fall_through_case(emu, oracle):
    O = oracle
    cid = 1
    bases = O.make_bases(cid, 33, KEY_N)
    sc = seeded_scalars(O, cid, 300, 7, "uniform")
    with emu.tuning(msm_compact=2, msm_wide=0, msm_wide_min=0):
        ck = emu.CommitmentKey(cid, bases)
        assert ck.is_compact() and not ck.has_wide_table() and ck.table_bytes() == 8 * KEY_N * 64
        assert np.array_equal(ck.commit(sc), O.msm(cid, sc, bases[:300]))
    ck.close()
    with emu.tuning(msm_compact=2):                          # the key-size rule: 1100 bases get no wide table
        ck = emu.CommitmentKey(cid, bases)
    assert ck.is_compact() and not ck.has_wide_table() and ck.table_bytes() == 8 * KEY_N * 64
    ck.close()
