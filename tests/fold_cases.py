"""The chunked commit with slot mode off, as a program for a test subprocess: shared by the emulator test and the GPU test."""


def bucket_fold_program(emu_lib=None):
    """Three-chunk streamed commits (the caller sets tuning msm_slots = 0, commit_chunks = 3) on both curves, uniform and trace-like
    scalars, against the oracle, then the key's statistics: six sets, none in slot mode, no redo.  `emu_lib`: path of the emulator
    build to load in place of the real library (None: the real library)."""
    load = f"from sirius_amd import _lib; _lib.load({emu_lib!r})\n" if emu_lib else ""
    return (
        "import sys, numpy as np; sys.path.insert(0, '.'); sys.path.insert(0, 'tests')\n"
        + load +
        "import sirius_amd as S, oracle as O\n"
        "from conftest import seeded_scalars\n"
        "n = 3000\n"
        "for cid in (0, 1):\n"
        "    bases = O.make_bases(cid, 7 + cid, n); ck = S.CommitmentKey(cid, bases)\n"
        "    for rep, kind in enumerate(('uniform', 'trace')):\n"
        "        sc = seeded_scalars(O, cid, n, 20 + rep, kind)\n"
        "        assert np.array_equal(ck.commit_upload(sc), O.msm(cid, sc, bases[:n])), (cid, rep, kind)\n"
        "    st = ck.msm_stats(); assert st['other_sets'] == 6 and st['slot_sets'] == 0 and st['redo'] == 0, st\n"
        "    ck.close()\n"
        "print('ok')\n")
