"""CPU: the bound audit of the sweep-form row programs.  The emitter (csrc/rowprog_compile.hip, emit_sweep_source) chains the 9 x 29-bit
primitives of csrc/field29.cuh lazily and decides from a static bound where a reducing product goes; the emulator's AUDIT build
(tests/emu/field29_audit.h: `make -C tests/emu audit`) carries the declared bounds next to the limbs and checks every primitive's stated
precondition on them.  The emitted code has no data-dependent branch, so one run of a program audits every operation of it.

For every program: reset the table, run the program through its sweep consumers, assert that no precondition was violated (and that
products were checked at all), and that the audited run's output equals the oracle -- the audit build computes what the real one does.
Programs: the stress gates of tests/sweep_stress_cases.py (each asserted to take its bookkeeping branch), every structure of
tests/golden/rowprog_programs.json in its recorded field, and the ahead-of-time programs (MainGate [5, 3] and [5]: cross terms with
d + 1 points, srs_eval_gates with one, the ProtoGalaxy leaf sweep on true and on reference leaf rows).  Inputs are the adversarial word
set; tests/test_sweep_bounds_gpu.py runs the same cases on the device.

The last tests run the word-set cases of the ahead-of-time kernels and the folds on the DEFAULT emulator library (the twins of the GPU
tests at k = 6 and k = 10)."""
import ctypes as C
import os
import subprocess

import pytest

from conftest import ROOT
import sweep_stress_cases as SC

EMU_DIR = os.path.join(ROOT, "tests", "emu")
KINDS = ["mul_value", "mul_limbs", "add_wrap", "sub_bound", "sub_limbs", "normalize", "reduce_range", "canonical_range", "pack_range",
         "untracked", "checked"]                 # f29_audit::Kind
SITE_BYTES = 160


def _session(target, name):
    """one emulator library for the tests of a module-scoped fixture.  The two fixtures below overlap in time (both are torn down at the
    end of the module, the later one first), so each end re-selects its OWN library before it undoes its tunables -- sirius_amd would
    otherwise load the product library to do so."""
    subprocess.check_call(["make", "-C", EMU_DIR, "-j8", target], stdout=subprocess.DEVNULL)
    import sirius_amd as S
    from sirius_amd import _lib
    path = os.path.join(EMU_DIR, name)
    _lib.load(path)
    old = os.environ.get("SRS_EMU_JIT")
    os.environ["SRS_EMU_JIT"] = "1"          # tests/emu/jit_emu.cpp compiles the emitted unit with g++ (with the shadows in the audit build)
    tun = S.tuning(jit_always=1)              # run-time compilation below k = 14 as well
    tun.__enter__()
    try:
        yield S
    finally:
        _lib.load(path)
        tun.__exit__(None, None, None)
        if old is None:
            os.environ.pop("SRS_EMU_JIT", None)
        else:
            os.environ["SRS_EMU_JIT"] = old
        _lib._lib = None                      # the real library is (re)loaded lazily by later tests


@pytest.fixture(scope="module")
def audit_emu():
    yield from _session("audit", "libsirius_emu_audit.so")


@pytest.fixture(scope="module")
def plain_emu():
    yield from _session("all", "libsirius_emu.so")


def read_audit(reset=True):
    """{kind: (count, first site)} of the kinds with a non-zero count"""
    from sirius_amd import _lib
    lib = _lib.lib()
    counts = (C.c_ulonglong * len(KINDS))()
    sites = C.create_string_buffer(len(KINDS) * SITE_BYTES)
    lib.srs_emu_f29_audit.restype = C.c_int
    lib.srs_emu_f29_audit.argtypes = [C.c_int, C.POINTER(C.c_ulonglong), C.c_char_p, C.c_int]
    assert lib.srs_emu_f29_audit(1 if reset else 0, counts, sites, len(KINDS)) == len(KINDS), "f29_audit::Kind and KINDS disagree"
    return {KINDS[k]: (counts[k], sites.raw[k * SITE_BYTES:(k + 1) * SITE_BYTES].split(b"\0")[0].decode()) for k in range(len(KINDS)) if counts[k]}


class audited:
    """with audited(what): the table is reset before the body and holds no violation after it (and at least one checked product)"""

    def __init__(self, what, expect_products=True):
        self.what, self.expect_products = what, expect_products

    def __enter__(self):
        read_audit()

    def __exit__(self, et, ev, tb):
        if et is not None:
            return False
        got = read_audit()
        checked = got.pop("checked", (0, ""))[0]
        assert not got, (self.what, "violated preconditions of the 9 x 29-bit primitives: {kind: (count, first site)}", got)
        assert checked > 0 or not self.expect_products, (self.what, "no product was audited")
        return False


def test_audit_library_shares_no_symbol_with_the_default_one(audit_emu):
    """Both emulator libraries live in one test process, and sizeof(f29_t) differs between them.  g++ marks the statics of inline
    functions and templates (the kernels' `__shared__` arrays) as process-unique symbols, which the dynamic linker unifies across
    libraries even under RTLD_LOCAL: the audit library is built with -fno-gnu-unique and must define none."""
    out = subprocess.check_output(["nm", "--defined-only", os.path.join(EMU_DIR, "libsirius_emu_audit.so")], text=True)
    unique = [line for line in out.splitlines() if line.split()[-2:-1] == ["u"]]
    assert not unique, unique[:5]


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c.name)
def test_audit_stress_gate(audit_emu, oracle, case):
    S = audit_emu
    with audited(case.name, expect_products=case.jit):
        SC.cross_case(S, oracle, case.field, 6, 0, case.nfix, case.nadv, case.gates, seed=7, kinds=(-2 if case.jit else -1, None))
    # the gate takes the bookkeeping branch it was built for (the emitted text does not depend on who runs it: no second compile)
    _, fixed, _, _ = SC.inputs(case.field, 0, case.nfix, case.nadv, 7)
    with S.tuning(no_jit=1):
        St = S.PlonkStructure(case.field, 6, [], fixed, case.nadv, case.gates)
    try:
        assert St.num_cross_terms == case.degree, (case.name, St.num_cross_terms)
        SC.check_marks(case, St)
    finally:
        St.close()


def _golden():
    import rowprog_cases
    return rowprog_cases.load()


@pytest.mark.parametrize("name", [e["name"] for e in _golden()])
def test_audit_recorded_structure(audit_emu, oracle, name):
    """the structures of tests/golden/rowprog_programs.json, each in its recorded field: the MainGate lists (ahead-of-time [5, 3] and [5],
    run-time compiled [3, 2] on Fq and [2, 5, 2]), the lookup structures (multi-round witnesses), the eight random circuits and the
    degree-10 structure (two passes of the interpreter: it has a sweep form that no kernel takes)"""
    S = audit_emu
    e = next(x for x in _golden() if x["name"] == name)
    if e["lookups"]:
        from lookup_cases import run_lookup_case
        with audited(name):
            run_lookup_case(S, oracle, name[len("lookup_"):], 5 if name.endswith("vector") else 4)
        return
    aot = name in ("main_gates_5_3", "main_gates_5")
    kind = "aot" if aot else (-2 if 1 <= e["degree"] <= 8 else -1)
    with audited(name, expect_products=kind != -1):
        n = SC.cross_case(S, oracle, e["field"], 6, e["num_selectors"], e["num_fixed"], e["num_advice"], e["gates"], seed=11, kinds=(kind, None))
    assert n == e["degree"]


@pytest.mark.parametrize("gate_T", [[5, 3], [5]], ids=["5_3", "5"])
def test_audit_ahead_of_time_one_point(audit_emu, oracle, gate_T):
    """sweep_kernel_body with d = 0: srs_eval_gates of the ahead-of-time programs, compressed and homogeneous"""
    with audited(f"eval_gates {gate_T}"):
        SC.eval_gates_case(audit_emu, oracle, 0, 6, gate_T, seed=12)


@pytest.mark.parametrize("compat", [False, True], ids=["true_rows", "reference_rows"])
def test_audit_protogalaxy_leaf_sweep(audit_emu, oracle, compat):
    """k_pg_leaves_sweep at k = 10, the smallest size that takes it: true leaf rows (eight accumulating leaves per thread with the folds
    between them); reference leaf rows under pg_compat_tree = 1 (the hoisting launch: the gates at row 0 once per gate and point), where
    prove's G starts at the point 2 (pt0 > 0)"""
    S = audit_emu
    with audited(f"protogalaxy leaves, reference_compat={compat}"):
        with S.tuning(pg_compat_tree=1 if compat else 0):
            SC.pg_case(S, oracle, 10, [5, 3], compat)


# ---- the twins of tests/test_sweep_bounds_gpu.py on the default emulator library (no run-time compilation here: tests/test_emu_jit.py
# compiles, and the audit build above runs every run-time compiled case on the same inputs)
@pytest.mark.parametrize("gate_T", [[5, 3], [5]], ids=["5_3", "5"])
def test_emu_word_set_ahead_of_time(plain_emu, oracle, gate_T):
    from workloads import gates_for
    gates, nfix, nadv = gates_for(gate_T)
    SC.cross_case(plain_emu, oracle, 0, 6, 0, nfix, nadv, gates, seed=11, kinds=("aot", None))
    SC.eval_gates_case(plain_emu, oracle, 0, 6, gate_T, seed=12)


@pytest.mark.parametrize("compat", [False, True], ids=["true_rows", "reference_rows"])
def test_emu_word_set_protogalaxy(plain_emu, oracle, compat):
    for gate_T in ([5, 3], [5]):
        SC.pg_case(plain_emu, oracle, 10, gate_T, compat)
    if compat:
        with plain_emu.tuning(pg_compat_tree=1):
            SC.pg_case(plain_emu, oracle, 10, [5, 3], compat)


@pytest.mark.parametrize("field", [0, 1])
def test_emu_word_set_folds(plain_emu, oracle, field):
    SC.fold_case(plain_emu, oracle, field)
