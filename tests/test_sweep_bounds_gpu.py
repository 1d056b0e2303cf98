"""GPU: the sweep-form row programs on adversarial words.  Every other row-program test draws its cells from workloads.rand_fe -- uniform
253-bit words: no word in [2^253, p) (a third of Fr), and lazy sums that stay near half their static bound.  Here every fixed, advice
and challenge word comes from tests/sweep_stress_cases.py's set (0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2, 2^253-1, 2^253, 2^232-1, one
uniform word) in a 64-row pattern with rows of all p-1, all 2^253-1 and all 0; expected values come from oracle.expr.cross_terms_oracle
and oracle.protogalaxy.  tests/test_sweep_bounds_emu.py audits the same programs' declared bounds on the emulator."""
import numpy as np
import pytest

import sweep_stress_cases as SC

pytestmark = pytest.mark.gpu

TILE = 256          # the run-time compiler takes structures from 2^14 rows on: the 64-row pattern 256 times (the oracle runs at 64 rows)


@pytest.fixture(scope="module")
def S():
    import sirius_amd
    return sirius_amd


@pytest.mark.parametrize("gate_T", [[5, 3], [5]], ids=["5_3", "5"])
def test_ahead_of_time_kernels(S, oracle, gate_T):
    """MainGate [5, 3] and [5] at k = 6: cross terms (d + 1 points) and srs_eval_gates (one point; homogeneous and compressed)"""
    from workloads import gates_for
    gates, nfix, nadv = gates_for(gate_T)
    SC.cross_case(S, oracle, 0, 6, 0, nfix, nadv, gates, seed=11, kinds=("aot", None))
    SC.eval_gates_case(S, oracle, 0, 6, gate_T, seed=12)


@pytest.mark.parametrize("field,gate_T", [(1, [3, 2]), (0, [2, 5, 2])], ids=["fq_3_2", "fr_2_5_2"])
def test_compiled_main_gates(S, oracle, field, gate_T):
    from workloads import gates_for
    gates, nfix, nadv = gates_for(gate_T)
    SC.cross_case(S, oracle, field, 6, 0, nfix, nadv, gates, seed=13, tile=TILE)


@pytest.mark.parametrize("case", SC.cases(), ids=lambda c: c.name)
def test_compiled_stress_gates(S, oracle, case):
    """each stress gate through the run-time compiled kernel (kind -2; the degree-9 gate stays on the interpreter) and under no_jit = 1"""
    n = SC.cross_case(S, oracle, case.field, 6, 0, case.nfix, case.nadv, case.gates, seed=7, tile=TILE, kinds=(-2 if case.jit else -1, -1))
    assert n == case.degree


def _random_circuits():
    import rowprog_cases
    return [e for e in rowprog_cases.load() if e["name"].startswith("random_")]


@pytest.mark.parametrize("name", [e["name"] for e in _random_circuits()])
def test_compiled_random_circuits(S, oracle, name):
    """the eight random circuits of tests/golden/rowprog_programs.json, evaluated on the device (tests/test_jit_gpu.py checks their hashes)"""
    e = next(x for x in _random_circuits() if x["name"] == name)
    n = SC.cross_case(S, oracle, e["field"], 6, e["num_selectors"], e["num_fixed"], e["num_advice"], e["gates"], seed=11, tile=TILE)
    assert n == e["degree"]


@pytest.mark.parametrize("compat", [True, False], ids=["reference_rows", "true_rows"])
@pytest.mark.parametrize("gate_T", [[5, 3], [5]], ids=["5_3", "5"])
def test_protogalaxy_leaf_sweep(S, oracle, gate_T, compat):
    """k = 10, the smallest size at which the leaf sweep is taken, one incoming trace: compute_G, evaluate_e, compute_F (and prove's K)"""
    SC.pg_case(S, oracle, 10, gate_T, compat)


def test_protogalaxy_reference_rows_hoisted_pass(S, oracle):
    """the reference's leaf rows through the hoisting launch of the leaf sweep (pg_compat_tree = 1) instead of the closed form"""
    with S.tuning(pg_compat_tree=1):
        SC.pg_case(S, oracle, 10, [5, 3], True)


@pytest.mark.parametrize("field", [0, 1])
def test_folds(S, oracle, field):
    """fold_witness, fold_error and fold_lincomb at n = 257"""
    SC.fold_case(S, oracle, field)
