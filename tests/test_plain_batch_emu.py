"""CPU: a set of MSMs on a plain commitment key as one linked flow (the segment is the pair (member, window)) on the emulator build of the
product kernels, against the oracle's MSM.  Form 1 on bn256 and form 2 on grumpkin, members of 600, 0 and 5 scalars on a 1024-base key.
Every case runs in a process of its own with the emulator library loaded (as test_plain_fold_emu does), so this file launches no emulated
kernel in the pytest process.  An emulated flow costs seconds whatever its size: one batch per case."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")
EMU_LIB = os.path.join(EMU_DIR, "libsirius_emu.so")


@pytest.fixture(scope="module")
def emu_built():
    subprocess.check_call(["make", "-C", EMU_DIR, "-j4"], stdout=subprocess.DEVNULL)


def _in_emulator(case, *args):
    code = ("import sys; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
            f"from sirius_amd import _lib; _lib.load({EMU_LIB!r})\n"
            "import oracle, sirius_amd, test_plain_batch_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid,form", [(0, 1), (1, 2)])
def test_emu_plain_batch(emu_built, cid, form):
    _in_emulator("_batch_case", cid, form)


def _batch_case(emu, oracle, cid, form):
    import plain_batch_cases as PB
    O = oracle
    bases = O.make_bases(cid, 1301 + cid, 1024)
    ck = PB.batch_key(emu, cid, form, bases)
    vs = PB.member_vectors(O, cid, (600, 0, 5), 1302)
    vs[2] = PB.mont(O, cid, [1, PB.PF.order(cid) - 1, 0x8000, 1 << 240, 0])       # the last member: digit and window boundaries
    got = PB.counted(ck, lambda: ck.commit_batch(vs), 1, 2, 2)
    assert np.array_equal(got, PB.oracle_batch(O, cid, vs, bases))
    assert not got[1].any()
    ck.close()
