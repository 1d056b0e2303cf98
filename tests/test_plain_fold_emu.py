"""CPU: streamed commits on plain commitment keys whose chunks fold their window buckets into the key's running buckets (one set per
window, one bucket reduction per commit) on the emulator build of the product kernels, against the oracle's MSM.  Form 1 on bn256 and
form 2 on grumpkin, each on a 3072-base key cut into three chunks.  Every case runs in a process of its own with the emulator library
loaded (as test_plain_glv_emu does), so this file launches no emulated kernel in the pytest process.  An emulated flow costs seconds
whatever its size: two commits per case."""
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
            "import oracle, sirius_amd, test_plain_fold_emu as T\n"
            f"T.{case}(sirius_amd, oracle, *{args!r}); print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0 and "ok" in r.stdout, (case, args, r.stdout[-300:], r.stderr[-1500:])


@pytest.mark.parametrize("cid,form", [(0, 1), (1, 2)])
def test_emu_plain_fold(emu_built, cid, form):
    _in_emulator("_fold_case", cid, form)


def _fold_case(emu, oracle, cid, form):
    from sirius_amd import _lib
    import plain_fold_cases as PF
    O = oracle
    lib = _lib.lib()
    bases = PF.degenerate_bases(O, lib, cid, form, 1101 + cid)      # bases[1024] = P, bases[2048] = -P (form 2: bases[1025] = phi(P))
    bases[2049] = bases[1]                                          # and an equal point in the first and the last chunk
    if form == 2:                                                   # bases[2050] = phi(bases[2]) = (beta x, y)
        import glv_cases as G
        lam, beta = G.constants(lib, cid)
        bf = O.BASE_FIELD[cid]
        bases[2050] = bases[2]
        bases[2050, :4] = O.fe_mul(bf, bases[2][None, :4], O.ints_to_mont(bf, [beta]))[0]
        assert O.is_on_curve(cid, bases[2050])
    ck = PF.fold_key(emu, cid, form, bases)
    # one vector: P of chunk 0 meets -P of chunk 2 in a running bucket (it returns to the identity), Q of chunk 0 meets Q of chunk 2 (the
    # fold's addition is a doubling), the middle chunk adds nothing
    fill = O.mont_to_ints(O.SCALAR_FIELD[cid], seeded_scalars(O, cid, PF.N_FULL, 1102, "uniform"))
    head = {0: 0x7FFF, 2048: 0x7FFF, 1: 0x8000, 2049: 0x8000}
    if form == 2:                                                   # a flagged entry of chunk 0 meets the unflagged same point of chunk 2
        head.update({2: lam * 1 % PF.order(cid), 2050: 1})
    sc = PF.zero_chunk(PF.with_head(O, cid, head, fill), 1)
    assert np.array_equal(PF.streamed(emu, ck, sc), O.msm(cid, sc, bases))
    tr = seeded_scalars(O, cid, PF.N_RAGGED, 1103, "trace")         # 1024 / 1024 / 5: the last set's buckets are all single
    assert np.array_equal(PF.streamed(emu, ck, tr), O.msm(cid, tr, bases[:PF.N_RAGGED]))
    ck.close()
