"""CPU: plain commitment keys (tuning msm_plain = 1: the bases alone) on the emulator build of the product kernels -- the window
grouping of the plain flow's segment passes, the 16 linked windows over the one table and the Horner chain that weights them, against the
oracle.  Every case runs in a process of its own with the emulator library loaded (as test_compact_wide_emu does), so this file launches
no emulated kernel in the pytest process.  An emulated flow of this kind costs seconds whatever its size: few commits."""
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
            "import oracle, sirius_amd, test_plain_key_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid", [0, 1])
def test_emu_plain_commit(emu_built, cid):
    _in_emulator("_commit_case", cid)


def test_emu_plain_streamed_and_batch(emu_built):
    _in_emulator("_streamed_and_batch_case")


def _commit_case(emu, oracle, cid):
    from oracle import pyref as P
    from plain_key_cases import boundary_ints, commit_counted, plain_key
    O = oracle
    bases = O.make_bases(cid, 41 + cid, KEY_N)
    ck = plain_key(emu, cid, bases)
    vals = boundary_ints(P.CURVES[cid].q)
    edge = np.concatenate([O.ints_to_mont(O.SCALAR_FIELD[cid], vals), seeded_scalars(O, cid, KEY_N - len(vals), 4, "uniform")])
    for sc in (edge, seeded_scalars(O, cid, KEY_N, 5, "trace"), seeded_scalars(O, cid, 1, 6, "uniform")):
        assert np.array_equal(commit_counted(ck, sc), O.msm(cid, sc, bases[:len(sc)])), len(sc)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    ck.close()
    full = emu.CommitmentKey(cid, bases)                     # the tunable unset: the key of every earlier release
    assert not full.is_plain() and full.table_bytes() == 16 * KEY_N * 64
    full.close()


def _streamed_and_batch_case(emu, oracle):
    from plain_key_cases import check_bookkeeping, plain_key
    O = oracle
    cid = 1
    bases = O.make_bases(cid, 47, KEY_N)
    ck = plain_key(emu, cid, bases)
    sc = seeded_scalars(O, cid, KEY_N, 7, "trace")
    before = ck.msm_stats()
    with emu.tuning(commit_chunks=3):
        assert np.array_equal(ck.commit_upload(sc), O.msm(cid, sc, bases))
    after = ck.msm_stats()
    assert after["other_sets"] > before["other_sets"] and after["slot_sets"] == before["slot_sets"], (before, after)
    vs = [seeded_scalars(O, cid, n, 8 + n, "uniform") for n in (300, 63, 1)]
    assert np.array_equal(ck.commit_batch(vs), np.stack([O.msm(cid, v, bases[:len(v)]) for v in vs]))
    ck.close()
    with emu.tuning(msm_plain=1):
        empty = emu.CommitmentKey(cid, bases[:0])
    check_bookkeeping(empty, 0)
    empty.close()
