"""Shared cases of the routes behind compute_F, compute_G and evaluate_e that no other test runs directly: the hoisted leaf
passes of the reference's leaf rows (`pg_compat_tree=1`: the polynomial tree of F, leaves + weighted reduce) next to the closed form, and the
intended leaf rows on a row-sharded structure.  MainGate lists as in test_fast_paths_equal_general_paths: [5, 3] is the ahead-of-time gate
set at k >= 10, [2] takes the interpreter; k = 11 has two 1024-leaf tiles per gate."""
import random

import numpy as np


def _inputs(k, gate_T, seed=3):
    from workloads import gates_for, rand_fe
    rows = 1 << k
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(seed)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    Ws = [rand_fe(rng, nadv * rows) for _ in range(2)]      # the accumulator's trace and one incoming trace
    return gates, nfix, nadv, fixed, Ws


def _oracle_structure(O, k, gate_T, nfix, nadv, fixed):
    from oracle import expr as OE
    from oracle import protogalaxy as OPG
    og, fo, ao = [], 0, 0
    for T in gate_T:
        og.append(OE.main_gate_expression(T, 0, fo, ao, nfix)); fo += 2 * T + 5; ao += T + 2
    oS = OPG.Structure(O, og, k, [], fixed, nadv, 0)
    return oS, oS.context(1)


def run_reference_rows_case(S, O, k, gate_T):
    """reference_compat=True: compute_F, compute_G and evaluate_e byte-equal in the default settings (closed form), under `pg_compat_tree=1`
    (F's polynomial tree, integer-point G and e through the hoisted leaf passes), under `pg_compat_tree=1, pg_f_eval=1, pg_g_fft=1` (F and G
    evaluated on the roots of unity and interpolated by the ifft) and under `pg_f_eval=1, pg_g_fft=1` alone (the closed form on the roots of
    unity); the default result equals the literal oracle."""
    from oracle import protogalaxy as OPG
    from oracle import pyref as P
    from sirius_amd import protogalaxy as PG
    gates, nfix, nadv, fixed, Ws = _inputs(k, gate_T)
    St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
    ctx = PG.PolyContext(St, 1)
    rnd = random.Random(1)
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    ints = lambda a: O.mont_to_ints(O.FR, a)
    betas_i = [rnd.randrange(P.FR) for _ in range(ctx.betas_count)]
    delta_i = rnd.randrange(P.FR)
    betas, delta = m(betas_i), m([delta_i])[0]

    def product():
        return dict(F=PG.compute_F(ctx, betas, delta, Ws[0]), G=PG.compute_G(ctx, betas, Ws), e=PG.evaluate_e_from_trace(ctx, betas, Ws[1]))

    default = product()
    others = {}
    with S.tuning(pg_compat_tree=1):
        others["pg_compat_tree"] = product()
        with S.tuning(pg_f_eval=1, pg_g_fft=1):
            others["pg_compat_tree, pg_f_eval, pg_g_fft"] = product()
    with S.tuning(pg_f_eval=1, pg_g_fft=1):
        others["pg_f_eval, pg_g_fft"] = product()
    for setting, got in others.items():
        for name in ("F", "G", "e"):
            assert np.array_equal(default[name], got[name]), f"{name}: default != {setting}"
    St.close()
    oS, octx = _oracle_structure(O, k, gate_T, nfix, nadv, fixed)
    assert ints(default["F"]) == OPG.compute_F(oS, octx, betas_i, delta_i, Ws[0], [], True), "compute_F"
    assert ints(default["G"]) == OPG.compute_G(oS, octx, betas_i, Ws, [[], []], True), "compute_G"
    assert ints(default["e"]) == [OPG.evaluate_e_from_trace(oS, octx, betas_i, Ws[1], [], True)], "evaluate_e"


def run_sharded_true_rows_case(S, O, k, world, gate_T, nonzero_ranks, whole_cache):
    """reference_compat=False on `set_shard(rank, world)`, every rank on a fresh structure handle: the ranks' F, G and e added mod p equal
    the unsharded call, which equals the oracle's *_fast restatement; `nonzero_ranks` ranks return a non-zero part -- rank 0 alone where a
    tile is smaller than a stripe (k < 10: rank 0 evaluates everything), else the ranks that own one of the 2^(k - 10) tiles per gate.
    `whole_cache`: the calling module's dict -- the unsharded result of a shape is computed and compared with the oracle once per library."""
    from oracle import protogalaxy as OPG
    from oracle import pyref as P
    from sirius_amd import protogalaxy as PG
    gates, nfix, nadv, fixed, Ws = _inputs(k, gate_T)
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    ints = lambda a: O.mont_to_ints(O.FR, np.ascontiguousarray(a).reshape(-1, 4))
    r = random.Random(4)
    betas_i = [r.randrange(P.FR) for _ in range(k + (len(gates) - 1).bit_length())]
    delta_i = r.randrange(P.FR)

    def calls(rank=None):
        St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
        if rank is not None:
            St.set_shard(rank, world)
        ctx = PG.PolyContext(St, 1)
        assert ctx.betas_count == len(betas_i)
        out = [ints(PG.compute_F(ctx, m(betas_i), m([delta_i])[0], Ws[0], reference_compat=False)),
               ints(PG.compute_G(ctx, m(betas_i), Ws, reference_compat=False)),
               ints(PG.evaluate_e_from_trace(ctx, m(betas_i), Ws[1], reference_compat=False))]
        St.close()
        return out

    key = (k, tuple(gate_T))
    if key not in whole_cache:
        whole = calls()
        oS, octx = _oracle_structure(O, k, gate_T, nfix, nadv, fixed)
        assert whole[0] == OPG.compute_F_fast(oS, octx, betas_i, delta_i, Ws[0], [], False), "compute_F"
        assert whole[1] == OPG.compute_G_fast(oS, octx, betas_i, Ws, [[], []], False), "compute_G"
        assert whole[2] == [OPG.evaluate_e_fast(oS, octx, betas_i, Ws[1], [], False)], "evaluate_e"
        whole_cache[key] = whole
    whole = whole_cache[key]
    total = [[0] * len(v) for v in whole]
    nonzero = []
    for rank in range(world):
        part = calls(rank)
        nonzero.append(any(any(v) for v in part))
        total = [[(a + b) % P.FR for a, b in zip(tv, pv)] for tv, pv in zip(total, part)]
    assert total == whole, "the ranks' parts do not add up to the unsharded result"
    if k < 10:
        assert nonzero == [True] + [False] * (world - 1), nonzero      # rank 0 evaluates everything
    elif world == 2:
        assert nonzero == [True, True], nonzero
    else:
        assert nonzero == [True, True] + [False] * (world - 2), nonzero      # two tiles per gate at k = 11: rank 2 owns none
    assert sum(nonzero) == nonzero_ranks
