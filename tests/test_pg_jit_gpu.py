"""GPU: ProtoGalaxy leaf kernels compiled at run time for any gate set (srs_structure_prepare_pg_leaves).  Every case uses the
intended leaf rows (reference_compat=False) on a structure with compiled leaf kernels and on a twin created under tuning(no_jit=1)
(tests/pg_jit_cases.py): kernel_kind(2) == 2 on the first, 0 on the twin, results byte-equal to each other and to the oracle.  The shapes
are the smallest that reach each branch of the three compiled kernels."""
import pytest

import pg_jit_cases as C

pytestmark = pytest.mark.gpu

_whole = {}


def test_one_tile_sweep_form(srs, oracle):
    """k = 10, [2], L = 1: one 1024-leaf tile per gate; sweep-form G at integer points (inside `prove`: F(alpha) stands for X = 1), sweep-form
    e, F's polynomial tree over the compiled leaf cubics"""
    C.run_main_gate_case(srs, oracle, 10, [2], 1)


def test_one_wave_bounds(srs, oracle):
    """the same shape with the unit bounded for one wave per SIMD (tuning pg_jit_waves=1: the choice for large gate programs)"""
    with srs.tuning(pg_jit_waves=1):
        C.run_main_gate_case(srs, oracle, 10, [2], 1)


def test_two_tiles_three_gates(srs, oracle):
    """k = 11, [2, 3, 2]: two tiles per gate, a fourth zero-padded gate block, the reduce across tiles"""
    C.run_main_gate_case(srs, oracle, 11, [2, 3, 2], 1)


def test_ten_points_run_form(srs, oracle):
    """k = 10, degree 9: 10 integer points > DMAX + 1, the `run` form per point"""
    C.run_high_degree_case(srs, oracle, 10, 9)


def test_three_incoming_traces(srs, oracle):
    """k = 10, [2], L = 3: G on the roots of unity, the witnesses folded through the coefficient table, `run` form"""
    C.run_main_gate_case(srs, oracle, 10, [2], 3)


def test_random_gate_with_selector_challenge_rotation(srs, oracle):
    C.run_random_gate_case(srs, oracle, 10)


@pytest.mark.parametrize("k", [10, 11])
def test_forced_against_ahead_of_time(srs, oracle, k):
    """[5, 3] under pg_jit_force=1: the compiled kernels against the ahead-of-time ones of the same gate set (the twin's kernel_kind is 1)"""
    C.run_main_gate_case(srs, oracle, k, [5, 3], 1, force=True)


def test_row_sharded(srs, oracle):
    """k = 11, [2], set_shard(rank, 2) for both ranks: tile ownership inside the shared body"""
    C.run_sharded_case(srs, oracle, 11, [2], 2, _whole)


def test_prepare_reports(srs, oracle):
    """return codes of prepare_pg_leaves: excluded structures say why (rc 10), an ahead-of-time gate set is 0 without a compile, and nothing
    is compiled at creation or by reference_compat calls"""
    import numpy as np
    from workloads import gates_for, rand_fe
    from sirius_amd import _lib, protogalaxy as PG
    rng = np.random.default_rng(1)

    def make(k, gate_T):
        gates, nfix, nadv = gates_for(gate_T)
        return srs.PlonkStructure(0, k, [], [rand_fe(rng, 1 << k, 0.3) for _ in range(nfix)], nadv, gates), nadv
    St, _ = make(8, [2])
    with pytest.raises(srs.SiriusAmdError) as e:
        St.prepare_pg_leaves()
    assert e.value.rc == _lib.ERR_UNSUPPORTED and "2^10" in str(e.value)
    St.close()
    St, nadv = make(10, [2])
    with srs.tuning(no_jit=1):
        with pytest.raises(srs.SiriusAmdError) as e:
            St.prepare_pg_leaves()
    assert e.value.rc == _lib.ERR_UNSUPPORTED and "no_jit" in str(e.value)
    # the reference's rows, and the intended rows below 2^14 rows, compile nothing
    with srs.tuning(jit_always=None):
        ctx = PG.PolyContext(St, 1)
        betas = rand_fe(rng, ctx.betas_count)
        W = rand_fe(rng, nadv << 10)
        PG.evaluate_e_from_trace(ctx, betas, W, reference_compat=True)
        PG.evaluate_e_from_trace(ctx, betas, W, reference_compat=False)
        assert St.kernel_kind(2) == 0
    with srs.tuning(jit_always=1):              # ... with jit_always the first call over the intended rows does
        lazy = PG.evaluate_e_from_trace(ctx, betas, W, reference_compat=False)
    assert St.kernel_kind(2) == 2 and St.prepare_pg_leaves() == 0.0
    with srs.tuning(no_jit=1):
        Si, _ = make(10, [2])
    # (same gates, other fixed columns: only the kinds are compared here)
    assert Si.kernel_kind(2) == 0 and lazy.shape == (4,)
    St.close(); Si.close()
    St, _ = make(10, [5, 3])
    assert St.kernel_kind(2) == 1 and St.prepare_pg_leaves() == 0.0 and St.kernel_kind(2) == 1
    St.close()
