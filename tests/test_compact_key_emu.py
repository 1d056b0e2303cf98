"""CPU: compact commitment keys (tuning msm_compact = 1: 8 stored windows + the curve endomorphism) on the emulator build of the
product kernels -- the split digits, the flagged payloads and the beta product in level 0, against the oracle.  Every case runs in a
process of its own with the emulator library loaded (as test_emu_two_pass_scatter does), so this file launches no emulated kernel in
the pytest process."""
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
            "import oracle, sirius_amd, test_compact_key_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid", [0, 1])
def test_emu_compact_commit(emu_built, cid):
    _in_emulator("_commit_case", cid)


def test_emu_compact_streamed_and_batched(emu_built):
    _in_emulator("_streamed_and_batched_case")


def _commit_case(emu, oracle, cid):
    O = oracle
    bases = O.make_bases(cid, 17 + cid, 1100)
    with emu.tuning(msm_compact=1):
        ck = emu.CommitmentKey(cid, bases)
    assert ck.is_compact() and ck.table_bytes() == 8 * 1100 * 64 and not ck.has_wide_table()
    for n, kind in ((300, "uniform"), (1100, "trace"), (1100, "uniform")):
        sc = seeded_scalars(O, cid, n, 5 + n, kind)
        assert np.array_equal(ck.commit(sc), O.msm(cid, sc, bases[:n])), (n, kind)
    assert np.array_equal(ck.bases(), bases) and ck.count_off_curve() == 0
    ck.close()
    with emu.tuning(msm_compact=1):
        empty = emu.CommitmentKey(cid, bases[:1024], rank=1, world=2)   # one stripe: rank 1 holds nothing, and is compact all the same
    assert empty.is_compact() and empty.table_bytes() == 0
    empty.close()
    full = emu.CommitmentKey(cid, bases)                    # the tunable unset: the key of every earlier release
    assert not full.is_compact() and full.table_bytes() == 16 * 1100 * 64
    sc = seeded_scalars(O, cid, 300, 6, "uniform")
    assert np.array_equal(full.commit(sc), O.msm(cid, sc, bases[:300]))
    full.close()


def _streamed_and_batched_case(emu, oracle):
    O = oracle
    cid = 1
    bases = O.make_bases(cid, 23, 1100)
    with emu.tuning(msm_compact=1):
        ck = emu.CommitmentKey(cid, bases)
    sc = seeded_scalars(O, cid, 1097, 5, "trace")
    want = O.msm(cid, sc, bases[:1097])
    with emu.tuning(commit_chunks=3):                       # several sets in slot mode, sliding base offsets
        assert np.array_equal(ck.commit_upload(sc), want)
    vs = [sc, seeded_scalars(O, cid, 300, 8, "uniform"), sc[:1]]
    for got, v in zip(ck.commit_batch(vs), vs):
        assert np.array_equal(got, O.msm(cid, v, bases[:len(v)]))
    st = ck.msm_stats()
    assert st["slot_sets"] >= 2 and st["other_sets"] >= 1, st
    ck.close()
