"""Shared cases of the closed-form ProtoGalaxy sums (reference_compat: every leaf of a gate is that gate at row 0, so the weighted sums
factor over the index bits -- DESIGN.md 4.4).  Every call is compared with the oracle's literal restatement (oracle/protogalaxy.py) and,
bit for bit, with the same call under `pg_compat_tree=1`, which sends it through the hoisted leaf passes and the weighted trees."""
import random

import numpy as np


def structure_gates(name):
    """-> (gates, nfix, nadv, num_challenges): `name` = 1 | 2 | 3 high-degree gates (degree 6 over MainGate<2>'s columns; three gates pad
    the table with a block of zero leaves), ("main", [T, ..]) MainGate<T> lists, or "primary+challenge": the Sangria primary's two gates
    (MainGate<5> + MainGate<3>) with a challenge factor each, so that compute_G folds the traces' challenges per evaluation point, or "deg2":
    one gate of degree 2 (three incoming traces: 8 points of G, a 256-point K domain)."""
    from sirius_amd import expression as X
    from workloads import gates_for, high_degree_gate, make_structure_inputs
    if name == "primary+challenge":
        w = make_structure_inputs("primary", 3, seed=1)
        nfix, nadv = w["num_fixed"], w["num_advice"]
        adv = lambda i: X.Polynomial(nfix + i)
        g0 = X.Sum(w["gates"][0], X.Product(X.Challenge(0), X.Product(adv(0), adv(1))))
        g1 = X.Sum(X.Product(X.Challenge(0), w["gates"][1]), adv(8))
        return [g0, g1], nfix, nadv, 1
    if name == "deg2":
        f, a = (lambda i: X.Polynomial(i)), (lambda i: X.Polynomial(2 + i))
        return [X.Sum(X.Sum(X.Product(X.Product(f(0), a(0)), a(1)), X.Product(f(1), a(0))), a(2))], 2, 3, 0
    if isinstance(name, tuple):
        gates, nfix, nadv = gates_for(name[1])
        return gates, nfix, nadv, 0
    T, n = 2, int(name)
    nfix, nadv = n * (2 * T + 5), n * (T + 2)
    return [high_degree_gate(T, 6, 0, g * (2 * T + 5), g * (T + 2), nfix) for g in range(n)], nfix, nadv, 0


def _oracle_gates(gates_name, gates, nfix):
    from oracle import expr as OE
    if isinstance(gates_name, tuple):
        og, fo, ao = [], 0, 0
        for T in gates_name[1]:
            og.append(OE.main_gate_expression(T, 0, fo, ao, nfix)); fo += 2 * T + 5; ao += T + 2
        return og
    return list(gates)          # the node tuples are the oracle's too


def run_closed_case(S, O, k, gates_name, L_traces, seed=5, ro=None):
    """compute_F, compute_G, evaluate_e and the one-call prove (given challenges, and with alpha / gamma squeezed from a PoseidonHash
    transcript -- `ro`, default: whenever K has 256 coefficients; the python sponge over 2^16 takes ~10 s) of one reference_compat case:
    closed form == weighted trees == oracle."""
    import torch
    from oracle import protogalaxy as OPG
    from oracle import pyref as P
    from sirius_amd import protogalaxy as PG
    from workloads import rand_fe
    rnd = random.Random(seed + 31 * k)
    rows = 1 << k
    gates, nfix, nadv, nch = structure_gates(gates_name)
    rng = np.random.default_rng(seed + k)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    Ws = [rand_fe(rng, nadv * rows) for _ in range(L_traces + 1)]
    St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
    ctx = PG.PolyContext(St, L_traces)
    oS = OPG.Structure(O, _oracle_gates(gates_name, gates, nfix), k, [], fixed, nadv, nch)
    octx = oS.context(L_traces)
    t = ctx.betas_count
    assert t == octx.betas_count() == k + (len(gates) - 1).bit_length()
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    ints = lambda a: O.mont_to_ints(O.FR, a)
    betas = [rnd.randrange(P.FR) for _ in range(t)]
    delta, alpha, gamma = (rnd.randrange(P.FR) for _ in range(3))
    chs_i = [[rnd.randrange(P.FR) for _ in range(nch)] for _ in Ws]
    chs = [m(c) if nch else np.zeros((0, 4), np.uint64) for c in chs_i]
    bs = OPG.beta_stroke(betas, alpha, delta)
    dWs = [torch.from_numpy(w.view(np.int64)).cuda() for w in Ws] if torch.cuda.is_available() else Ws    # device-resident (emulator: host)
    logK = octx.fft_log_domain_size_K()
    ro = logK <= 8 if ro is None else ro

    def product():
        out = dict(F=PG.compute_F(ctx, m(betas), m([delta])[0], Ws[0], challenges=chs[0]),
                   G=PG.compute_G(ctx, m(bs), Ws, challenges_list=chs),
                   e=PG.evaluate_e_from_trace(ctx, m(bs), Ws[-1], challenges=chs[-1]))
        if logK <= P.FR_S:
            pr = PG.prove(ctx, m(betas), m([delta])[0], dWs, alpha=m([alpha])[0], gamma=m([gamma])[0], challenges_list=chs, fold=False)
            out.update({"prove." + n: pr[n] for n in ("poly_F", "poly_K", "alpha", "gamma", "e", "betas_stroke", "lagrange")})
            if ro:
                h = S.PoseidonHash(0, 5, 4, 10, 10)
                h.absorb_field(m([delta]))
                pr = PG.prove(ctx, m(betas), m([delta])[0], dWs, ro=h, challenges_list=chs, fold=False)
                out.update({"prove_ro." + n: pr[n] for n in ("poly_F", "poly_K", "alpha", "gamma", "e", "betas_stroke", "lagrange")})
        return out

    closed = product()
    with S.tuning(pg_compat_tree=1):
        tree = product()
    assert closed.keys() == tree.keys()
    for name in closed:
        assert np.array_equal(closed[name], tree[name]), f"closed form != weighted trees: {name}"
    # ---- the literal oracle
    eF = OPG.compute_F(oS, octx, betas, delta, Ws[0], chs_i[0], True)
    assert ints(closed["F"]) == eF, "compute_F"
    eG = OPG.compute_G(oS, octx, bs, Ws, chs_i, True)
    assert ints(closed["G"]) == eG, "compute_G"
    assert ints(closed["e"]) == [OPG.evaluate_e_from_trace(oS, octx, bs, Ws[-1], chs_i[-1], True)], "evaluate_e"
    if logK <= P.FR_S:
        Fa = OPG.poly_eval(eF, alpha)
        eK = OPG.compute_K_from_G(octx, eG, Fa)
        Lg = P.eval_lagrange_poly_for_cyclic_group(gamma, octx.lagrange_domain())
        assert ints(closed["prove.poly_F"]) == eF and ints(closed["prove.poly_K"]) == eK, "prove: F, K"
        assert ints(closed["prove.alpha"]) == [alpha] and ints(closed["prove.gamma"]) == [gamma]
        assert ints(closed["prove.betas_stroke"]) == bs and ints(closed["prove.lagrange"]) == Lg[: len(Ws)]
        assert ints(closed["prove.e"]) == [OPG.calculate_e(eF, eK, gamma, alpha, octx.lagrange_domain())], "prove: e"
        if ro:
            from oracle import poseidon as OP
            oro = OP.PoseidonHash(P.FR, 5, 4, 10, 10)
            oro.absorb_field_iter([delta])
            a2 = oro.absorb_field_iter(eF).squeeze(255)
            assert ints(closed["prove_ro.alpha"]) == [a2] and ints(closed["prove_ro.poly_F"]) == eF
            bs2 = OPG.beta_stroke(betas, a2, delta)
            eK2 = OPG.compute_K_from_G(octx, OPG.compute_G(oS, octx, bs2, Ws, chs_i, True), OPG.poly_eval(eF, a2))
            g2 = oro.absorb_field_iter(eK2).squeeze(255)
            assert ints(closed["prove_ro.poly_K"]) == eK2 and ints(closed["prove_ro.gamma"]) == [g2]
            assert ints(closed["prove_ro.betas_stroke"]) == bs2
            assert ints(closed["prove_ro.lagrange"]) == P.eval_lagrange_poly_for_cyclic_group(g2, octx.lagrange_domain())[: len(Ws)]
            assert ints(closed["prove_ro.e"]) == [OPG.calculate_e(eF, eK2, g2, a2, octx.lagrange_domain())]
    St.close()
    return ctx


def run_sharded_case(S, O, k, gates_name, world, seed=6):
    """`set_shard(r, w)`: the ranks' partial F, G and e add up to the unsharded result; ranks >= 1 return zeros (there is nothing to shard
    when every leaf reads row 0)."""
    from oracle import pyref as P
    from sirius_amd import protogalaxy as PG
    from workloads import rand_fe
    rnd = random.Random(seed + k)
    rows = 1 << k
    gates, nfix, nadv, _ = structure_gates(gates_name)
    rng = np.random.default_rng(seed + k)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    Ws = [rand_fe(rng, nadv * rows) for _ in range(2)]
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    ints = lambda a: O.mont_to_ints(O.FR, np.ascontiguousarray(a).reshape(-1, 4))

    def calls(St):
        ctx = PG.PolyContext(St, 1)
        r = random.Random(seed)
        betas = m([r.randrange(P.FR) for _ in range(ctx.betas_count)])
        delta = m([r.randrange(P.FR)])[0]
        return [ints(PG.compute_F(ctx, betas, delta, Ws[0])), ints(PG.compute_G(ctx, betas, Ws)), ints(PG.evaluate_e_from_trace(ctx, betas, Ws[1]))]

    St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
    whole = calls(St)
    St.close()
    assert any(whole[0]) and any(whole[1]) and any(whole[2])
    total = [[0] * len(v) for v in whole]
    for rank in range(world):
        St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
        St.set_shard(rank, world)
        part = calls(St)
        St.close()
        if rank:
            assert not any(any(v) for v in part), f"rank {rank} of {world} must return zeros"
        total = [[(a + b) % P.FR for a, b in zip(tv, pv)] for tv, pv in zip(total, part)]
    assert total == whole
