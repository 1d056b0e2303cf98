"""CPU: the ProtoGalaxy leaf kernels compiled at run time, end to end on the logic emulator: the library emits the leaf unit of a gate set
exactly as it does for hiprtc (pg_leaf_unit_source: the per-gate programs, the dispatcher, three kernels over the bodies of
rowprog_dev.cuh), tests/emu/jit_emu_units.h compiles that text with g++ and enters each kernel through its launcher.  The cases of
tests/pg_jit_cases.py that need no GPU-sized table; one of them again on the audit library (field29_audit.h), where the eight leaves of a
thread accumulate into the same lazy 9 x 29-bit sums."""
import ctypes as C
import os
import subprocess

import pytest

import pg_jit_cases as cases
from conftest import ROOT

EMU_DIR = os.path.join(ROOT, "tests", "emu")


def _loaded(lib_name, make_target):
    subprocess.check_call(["make", "-C", EMU_DIR, "-j4"] + make_target, stdout=subprocess.DEVNULL)
    import sirius_amd as S
    from sirius_amd import _lib
    _lib.load(os.path.join(EMU_DIR, lib_name))
    old = os.environ.get("SRS_EMU_JIT")
    os.environ["SRS_EMU_JIT"] = "1"          # tests/emu/jit_emu.cpp: compile the emitted source with g++ (the emulator's stand-in for hiprtc)
    try:
        yield S
    finally:
        if old is None:
            os.environ.pop("SRS_EMU_JIT", None)
        else:
            os.environ["SRS_EMU_JIT"] = old
        _lib._lib = None


@pytest.fixture(scope="module")
def emu_jit():
    yield from _loaded("libsirius_emu.so", [])


@pytest.fixture(scope="module")
def emu_audit():
    yield from _loaded("libsirius_emu_audit.so", ["audit"])


def test_emu_one_tile_sweep_form(emu_jit, oracle):
    cases.run_main_gate_case(emu_jit, oracle, 10, [2], 1)


def test_emu_two_tiles_three_gates(emu_jit, oracle):
    cases.run_main_gate_case(emu_jit, oracle, 11, [2, 3, 2], 1)


def test_emu_ten_points_run_form(emu_jit, oracle):
    cases.run_high_degree_case(emu_jit, oracle, 10, 9)


def test_emu_random_gate(emu_jit, oracle):
    cases.run_random_gate_case(emu_jit, oracle, 10)


def test_emu_prepare_reports(emu_jit):
    """what excludes a structure is reported, and a unit the compiler rejects leaves the interpreter in place"""
    import numpy as np
    from sirius_amd import _lib
    from workloads import gates_for, rand_fe
    S = emu_jit
    rng = np.random.default_rng(2)
    gates, nfix, nadv = gates_for([2])
    St = S.PlonkStructure(0, 8, [], [rand_fe(rng, 256, 0.3) for _ in range(nfix)], nadv, gates)
    with pytest.raises(S.SiriusAmdError) as e:
        St.prepare_pg_leaves()
    assert e.value.rc == _lib.ERR_UNSUPPORTED and "2^10" in str(e.value) and St.kernel_kind(2) == 0
    St.close()
    St = S.PlonkStructure(1, 10, [], [rand_fe(rng, 1024, 0.3) for _ in range(nfix)], nadv, gates)      # Fq: no ProtoGalaxy
    with pytest.raises(S.SiriusAmdError) as e:
        St.prepare_pg_leaves()
    assert e.value.rc == _lib.ERR_UNSUPPORTED and "Fr" in str(e.value)
    St.close()
    # above the cap (16 gates, 608 SSA instructions > 320): refused with the count, nothing compiled, and the leaves run on the
    # interpreter -- the same value as on a twin that may not compile at all
    from sirius_amd import protogalaxy as PG
    gates, nfix, nadv = gates_for([2, 3] * 8)
    fixed = [rand_fe(rng, 1024, 0.3) for _ in range(nfix)]
    W = rand_fe(rng, nadv * 1024)
    St = S.PlonkStructure(0, 10, [], fixed, nadv, gates)
    with pytest.raises(S.SiriusAmdError) as e:
        St.prepare_pg_leaves()
    assert e.value.rc == _lib.ERR_UNSUPPORTED and "608 instructions" in str(e.value) and "320" in str(e.value), str(e.value)
    ctx = PG.PolyContext(St, 1)
    betas = rand_fe(rng, ctx.betas_count)
    with S.tuning(jit_always=1):
        got = PG.evaluate_e_from_trace(ctx, betas, W, reference_compat=False)
    assert St.kernel_kind(2) == 0
    with S.tuning(no_jit=1):
        Si = S.PlonkStructure(0, 10, [], fixed, nadv, gates)
        want = PG.evaluate_e_from_trace(PG.PolyContext(Si, 1), betas, W, reference_compat=False)
    assert np.array_equal(got, want)
    St.close(); Si.close()


def test_emu_audit_leaf_accumulation(emu_audit, oracle):
    """shape 1 on the audit build: the compiled sweep-form leaf kernel violates no precondition of the 9 x 29-bit form"""
    from sirius_amd import _lib
    lib = _lib.lib()
    lib.srs_emu_f29_audit.restype = C.c_int
    lib.srs_emu_f29_audit.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_char_p, C.c_int]
    kinds = lib.srs_emu_f29_audit(1, None, None, 0)
    cases.run_main_gate_case(emu_audit, oracle, 10, [2], 1)
    counts = (C.c_ulonglong * kinds)()
    sites = C.create_string_buffer(kinds * 160)
    assert lib.srs_emu_f29_audit(1, counts, sites, kinds) == kinds
    from test_sweep_bounds_emu import KINDS
    assert kinds == len(KINDS)
    got = {KINDS[i]: (counts[i], sites.raw[i * 160:(i + 1) * 160].split(b"\0")[0].decode()) for i in range(kinds) if counts[i]}
    checked = got.pop("checked", (0, ""))[0]                # not a violation: the number of products whose precondition was checked
    assert not got, ("violated preconditions of the 9 x 29-bit primitives: {kind: (count, first site)}", got)
    assert checked > 0, "no product was audited"
