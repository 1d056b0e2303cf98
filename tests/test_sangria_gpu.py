"""GPU parity: Sangria prover row work through the C-ABI vs the oracle's literal restatement
(GroupedPoly terms + GraphEvaluator interpreter): commit_cross_terms (src/nifs/sangria/mod.rs:102-158),
RelaxedPlonkWitness::fold (accumulator.rs:364-404), decider gate values.  Bit-exact."""
import numpy as np
import pytest

from oracle import expr as OE
from oracle import pyref as P
from workloads import gates_for, make_structure_inputs

pytestmark = pytest.mark.gpu


def _oracle_gates(gate_T):
    nfix = sum(2 * T + 5 for T in gate_T)
    gates, fo, ao = [], 0, 0
    for T in gate_T:
        gates.append(OE.main_gate_expression(T, 0, fo, ao, nfix))
        fo += 2 * T + 5
        ao += T + 2
    return gates


@pytest.mark.parametrize("which,k,gate_T", [("primary", 10, [5, 3]), ("secondary", 10, [5]), ("primary", 6, [2]),
                                            ("secondary", 7, [3, 2, 2]), ("primary", 13, [5, 3]), ("secondary", 13, [5])])
def test_commit_cross_terms_vs_oracle(srs, oracle, which, k, gate_T):
    O = oracle
    w = make_structure_inputs(which, k, seed=k * 31 + len(gate_T))
    field, curve, rows = w["field"], w["curve"], w["rows"]
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(k)
    from workloads import rand_fe, trace_like
    fixed = [rand_fe(rng, rows, 0.5) for _ in range(nfix)]
    W1, W2 = trace_like(rng, nadv * rows), rand_fe(rng, nadv * rows)
    S = srs.PlonkStructure(field, k, [], fixed, nadv, gates)
    nch = S.num_challenges
    u1c, u1u, u2c = rand_fe(rng, nch), rand_fe(rng, 1)[0], rand_fe(rng, nch)
    bases = O.make_bases(curve, 77, rows)
    ck = srs.CommitmentKey(curve, bases)
    terms, commits = srs.VanillaFS.commit_cross_terms(ck, S, u1c, u1u, W1, u2c, W2)
    ch = srs.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    cg, exp = OE.cross_terms_oracle(O, field, _oracle_gates(gate_T), 0, nfix, nadv, [], fixed, W1, W2, ch)
    assert S.num_cross_terms == cg.degree == len(exp) and nch == cg.num_challenges_compressed
    for i, (a, b) in enumerate(zip(terms, exp)):
        assert np.array_equal(a, b), ("cross term", i)
        assert np.array_equal(commits[i], O.msm(curve, b, bases)), ("commit", i)     # src/nifs/sangria/mod.rs:151-154
    # fold (accumulator.rs:364-404)
    r, E = rand_fe(rng, 1)[0], rand_fe(rng, rows)
    acc = srs.RelaxedPlonkWitness(field, [W1], E).fold([W2], terms, r)
    assert np.array_equal(acc.W[0], O.fold_w(field, W1, W2, r))
    assert np.array_equal(acc.E, O.fold_e(field, E, exp, r))
    # deciders' per-row gate values (plonk/mod.rs:328, sangria/mod.rs:351)
    p = P.MODULI[field]
    pc = OE.GraphEvaluator(cg.compressed, p).export(field, O)
    assert np.array_equal(S.eval_gates(W1, u1c), O.eval_program(field, pc, [], fixed, W1, W2, u1c.reshape(-1, 4)))
    ph = OE.GraphEvaluator(cg.homogeneous, p).export(field, O)
    chh = np.concatenate([u1c.reshape(-1, 4), u1u.reshape(1, 4)])
    assert np.array_equal(S.eval_gates(W1, chh, homogeneous=True), O.eval_program(field, ph, [], fixed, W1, W2, chh))


def test_selectors_rotations_constants(srs, oracle):
    """Selector columns (bool -> 0/1), rotations that wrap (graph_evaluator.rs:51-53), constants, negation, scaling."""
    O = oracle
    from sirius_amd import expression as X
    from workloads import rand_fe
    field, k = 0, 5
    rows = 1 << k
    rng = np.random.default_rng(3)
    nsel, nfix, nadv = 2, 2, 3
    px = [X.Sum(X.Product(X.Polynomial(0), X.Sum(X.Polynomial(4, 1), X.Negated(X.Polynomial(5, -1)))),
                X.Scaled(X.Product(X.Polynomial(6, rows - 1), X.Polynomial(6, rows - 1)), 7)),
          X.Sum(X.Product(X.Polynomial(1), X.Product(X.Polynomial(2, -3), X.Polynomial(4))), X.Negated(X.Constant(5))),
          X.Product(X.Sum(X.Polynomial(3), X.Constant(2)), X.Polynomial(5, 2))]
    ox = [OE.Sum(OE.Prod(OE.Poly(0), OE.Sum(OE.Poly(4, 1), OE.Neg(OE.Poly(5, -1)))), OE.Scaled(OE.Prod(OE.Poly(6, rows - 1), OE.Poly(6, rows - 1)), 7)),
          OE.Sum(OE.Prod(OE.Poly(1), OE.Prod(OE.Poly(2, -3), OE.Poly(4))), OE.Neg(OE.Const(5))),
          OE.Prod(OE.Sum(OE.Poly(3), OE.Const(2)), OE.Poly(5, 2))]
    sel = [rng.integers(0, 2, size=rows, dtype=np.uint8) for _ in range(nsel)]
    fixed = [rand_fe(rng, rows) for _ in range(nfix)]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    S = srs.PlonkStructure(field, k, sel, fixed, nadv, px)
    nch = S.num_challenges
    u1c, u1u, u2c = rand_fe(rng, nch), rand_fe(rng, 1)[0], rand_fe(rng, nch)
    terms, _ = srs.VanillaFS.commit_cross_terms(None, S, u1c, u1u, W1, u2c, W2)
    ch = srs.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    cg, exp = OE.cross_terms_oracle(O, field, ox, nsel, nfix, nadv, sel, fixed, W1, W2, ch)
    assert len(terms) == len(exp) == cg.degree
    for a, b in zip(terms, exp):
        assert np.array_equal(a, b)


def test_structure_errors(srs):
    from sirius_amd import expression as X
    from workloads import rand_fe
    rng = np.random.default_rng(1)
    with pytest.raises(srs.SiriusAmdError) as e:       # query index beyond the advice columns (eval.rs:3-25)
        srs.PlonkStructure(0, 3, [], [rand_fe(rng, 8)], 1, [X.Product(X.Polynomial(0), X.Polynomial(5))])
    assert e.value.rc == 7


def test_fold_step_device_resident_k17_properties(srs, oracle):
    """Full-size (k=17) primary prover step on HBM-resident data, checked through size-independent
    properties: (1) homomorphism  commit(W1 + r W2) == C1 + [r] C2; (2) the cross terms satisfy
    P_hom(W_fold, ch_fold) == P_hom(W1,ch1) + sum_k r^k T_k  per row (definition of T_k), evaluated by
    the decider program on the folded witness; sampled rows are checked against the oracle."""
    import torch
    O = oracle
    w = make_structure_inputs("primary", 17, seed=2024)
    field, curve, rows, nadv = w["field"], w["curve"], w["rows"], w["num_advice"]
    S = srs.PlonkStructure(field, 17, [], w["fixed"], nadv, w["gates"])
    bases = O.make_bases(curve, 5, nadv * rows)
    ck = srs.CommitmentKey(curve, bases)
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    W1, W2, E = dev(w["W1"]), dev(w["W2"]), dev(w["E"])
    terms, commits = srs.VanillaFS.commit_cross_terms(ck, S, w["u1_challenges"], w["u1_u"], W1, w["u2_challenges"], W2)
    r = w["r"]
    acc = srs.RelaxedPlonkWitness(field, [W1], E).fold([W2], terms, r)
    # (1)
    c1, c2, cf = ck.commit(W1), ck.commit(W2), ck.commit(acc.W[0])
    assert np.array_equal(cf, srs.point_sum(curve, np.stack([c1, srs.point_mul(curve, r, c2)])))
    # (2) P_hom(fold) - P_hom(W1) == sum r^k T_k  <=> E' - E (with E := P_hom(W1) stand-in) ; use fold_error on zeros
    ch1 = np.concatenate([w["u1_challenges"].reshape(-1, 4), w["u1_u"].reshape(1, 4)])
    one = srs.field.to_mont(field, 1)
    ch2 = np.concatenate([w["u2_challenges"].reshape(-1, 4), one.reshape(1, 4)])
    chf = O.fe_add(field, ch1, O.fe_mul(field, np.broadcast_to(r, ch2.shape).copy(), ch2))
    p0 = S.eval_gates(W1, ch1, homogeneous=True)
    pf = S.eval_gates(acc.W[0], chf, homogeneous=True)
    rhs = srs.RelaxedPlonkWitness(field, [], p0).fold([], terms, r).E
    assert torch.equal(pf, rhs)
    # sampled rows of T_k against the oracle on a row-subsampled instance is not possible (rotations are 0 here):
    # restrict every column to the first 256 rows and recompute with the oracle
    sub = 256
    from oracle import expr as OE2
    fixed_s = [f[:sub] for f in w["fixed"]]
    w1s = np.concatenate([w["W1"][c * rows: c * rows + sub] for c in range(nadv)])
    w2s = np.concatenate([w["W2"][c * rows: c * rows + sub] for c in range(nadv)])
    ch = srs.VanillaFS.cross_term_challenges(w["u1_challenges"], w["u1_u"], w["u2_challenges"], field)
    _, exp = OE2.cross_terms_oracle(O, field, _oracle_gates([5, 3]), 0, w["num_fixed"], nadv, [], fixed_s, w1s, w2s, ch)
    for t, e in zip(terms, exp):
        assert np.array_equal(t[:sub].cpu().numpy().view(np.uint64), e)
    assert np.array_equal(commits[0], O.msm(curve, terms[0].cpu().numpy().view(np.uint64), bases[:rows]))


@pytest.mark.parametrize("which,seed", [("primary", 2), ("secondary", 3)])
def test_sangria_config_k17_vs_oracle(srs, oracle, which, seed):
    """BASELINE configs[1] at FULL size, directly against the oracle (VanillaFS::commit_cross_terms, src/nifs/sangria/mod.rs:102-158):
    all 6 (primary, bn256) / 5 (secondary, grumpkin) cross-term vectors of 2^17 rows and their commitments over the bench's own
    2^21 key == the literal GroupedPoly + GraphEvaluator oracle and best_multiexp; then the witness / error folds."""
    import os
    import torch
    from workloads import sangria_shape
    O = oracle
    threads = min(32, 2 * (len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 8))
    k = 17
    w = make_structure_inputs(which, k, seed=0x5349524955530000 + seed)            # bench.py's extras_sangria inputs
    field, curve, rows, nadv = w["field"], w["curve"], w["rows"], w["num_advice"]
    S = srs.PlonkStructure(field, k, [], w["fixed"], nadv, w["gates"])
    ck = srs.CommitmentKey.setup_synthetic(curve, 1 << 21, seed=42 + curve)
    bases = ck.bases()
    dev = lambda a: torch.from_numpy(a.view(np.int64)).cuda()
    W1, W2, E = dev(w["W1"]), dev(w["W2"]), dev(w["E"])
    terms, commits = srs.VanillaFS.commit_cross_terms(ck, S, w["u1_challenges"], w["u1_u"], W1, w["u2_challenges"], W2)
    ch = srs.VanillaFS.cross_term_challenges(w["u1_challenges"], w["u1_u"], w["u2_challenges"], field)
    cg, exp = OE.cross_terms_oracle(O, field, _oracle_gates(sangria_shape(which)["gate_T"]), 0, w["num_fixed"], nadv, [], w["fixed"],
                                    w["W1"], w["W2"], ch, threads)
    assert len(terms) == len(exp) == cg.degree == (6 if which == "primary" else 5)
    for i, (t, e) in enumerate(zip(terms, exp)):
        assert np.array_equal(t.cpu().numpy().view(np.uint64), e), f"{which}: cross term {i + 1}"
        assert np.array_equal(commits[i], O.msm(curve, e, bases[:rows], threads)), f"{which}: commitment of cross term {i + 1}"
    acc = srs.RelaxedPlonkWitness(field, [W1], E).fold([W2], terms, w["r"])
    assert np.array_equal(acc.W[0].cpu().numpy().view(np.uint64), O.fold_w(field, w["W1"], w["W2"], w["r"], threads))
    assert np.array_equal(acc.E.cpu().numpy().view(np.uint64), O.fold_e(field, w["E"], exp, w["r"], threads))
    assert np.array_equal(ck.commit(W2), O.msm(curve, w["W2"], bases[: nadv * rows], threads))
    S.close(); ck.close()


def _is_sat_case(S, O, field=0, k=6, gate_T=(5, 3)):
    """Deciders' gate check (src/plonk/mod.rs:329-346, src/nifs/sangria/mod.rs:352-376): mismatch counts vs the oracle."""
    from workloads import rand_fe
    gate_T = list(gate_T)
    rows = 1 << k
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(12)
    fixed = [rand_fe(rng, rows, 0.5) for _ in range(nfix)]
    W = rand_fe(rng, nadv * rows)
    W.reshape(nadv, rows, 4)[:, : rows // 4] = 0            # rows where every advice cell is 0
    for f in fixed[-1:] + fixed[2 * gate_T[0] + 4: 2 * gate_T[0] + 5]:
        f[: rows // 4] = 0                                   # rc columns zero there -> those rows satisfy the gates
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    nch = St.num_challenges
    uc, uu = rand_fe(rng, nch), rand_fe(rng, 1)[0]
    ctx = OE.QueryIndexContext(0, nfix, nadv, 0, 0)
    cg = OE.CompressedGates.new(_oracle_gates(gate_T), ctx)
    p = P.MODULI[field]
    comp = O.eval_program(field, OE.GraphEvaluator(cg.compressed, p).export(field, O), [], fixed, W, W, uc.reshape(-1, 4))
    exp = int(np.count_nonzero(np.any(comp != 0, axis=1)))
    assert St.is_sat_gates(W, uc) == exp and 0 < exp <= rows - rows // 4
    chh = np.concatenate([uc.reshape(-1, 4), uu.reshape(1, 4)])
    hom = O.eval_program(field, OE.GraphEvaluator(cg.homogeneous, p).export(field, O), [], fixed, W, W, chh)
    E = hom.copy()
    assert St.is_sat_gates(W, chh, E) == 0                   # E == P_hom(W, u): relaxed instance satisfied
    E[::3] = rand_fe(rng, len(E[::3]))
    assert St.is_sat_gates(W, chh, E) == len(E[::3])
    St.close()


def test_is_sat_gates(srs, oracle):
    _is_sat_case(srs, oracle, 0, 6, (5, 3))
    _is_sat_case(srs, oracle, 1, 9, (5,))


def _satisfying_witness(O, field, k, gate_T, fixed, rng):
    """Advice values that satisfy every MainGate<T> of the structure on every row: random state/input cells, and
    `out` solved from the gate (q_o is forced to 1).  Returns W (num_advice * rows, Montgomery)."""
    from workloads import rand_fe
    p = P.MODULI[field]
    rows = 1 << k
    nadv = sum(T + 2 for T in gate_T)
    Wi = [O.mont_to_ints(field, rand_fe(rng, rows)) for _ in range(nadv)]
    Fi = [O.mont_to_ints(field, f) for f in fixed]
    fo = ao = 0
    for T in gate_T:
        q1, q5 = Fi[fo:fo + T], Fi[fo + T:fo + 2 * T]
        qm, qi, qo, rc = Fi[fo + 2 * T:fo + 2 * T + 2], Fi[fo + 2 * T + 2], Fi[fo + 2 * T + 3], Fi[fo + 2 * T + 4]
        st, inp = Wi[ao:ao + T], Wi[ao + T]
        out = []
        for r in range(rows):
            acc = qm[0][r] * st[0][r] * st[1][r] + qi[r] * inp[r] + rc[r]
            if T >= 4:
                acc += qm[1][r] * st[2][r] * st[3][r]
            for i in range(T):
                acc += q1[i][r] * st[i][r] + q5[i][r] * pow(st[i][r], 5, p)
            assert qo[r] == 1
            out.append((-acc) % p)
        Wi[ao + T + 1] = out
        fo += 2 * T + 5
        ao += T + 2
    return O.ints_to_mont(field, [v for col in Wi for v in col])


def _fold_then_decide(S, O, field, curve, k, gate_T):
    """The reference's protocol tests (src/nifs/sangria/tests.rs:256-346) in miniature: fold a satisfying fresh
    instance into a satisfying accumulator, then run the decider's checks on the result:
      gate check  P_hom(W', u')[row] == E'[row]        (is_sat_accumulation, sangria/mod.rs:352-376)
      commitments commit(W') == C_W1 + r C_W2,  commit(E') == C_E + sum r^k C_Tk   (is_sat_witness_commit :455-474)"""
    from workloads import rand_fe
    gate_T = list(gate_T)
    rows = 1 << k
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(k * 3 + len(gate_T))
    fixed = [rand_fe(rng, rows, 0.2) for _ in range(nfix)]
    fo = 0
    one = O.ints_to_mont(field, [1])[0]
    for T in gate_T:                       # q_o := 1 so that `out` can be solved for
        fixed[fo + 2 * T + 3][:] = one
        fo += 2 * T + 5
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    nch = St.num_challenges
    y1, y2 = rand_fe(rng, nch), rand_fe(rng, nch)
    W1 = _satisfying_witness(O, field, k, gate_T, fixed, rng)
    W2 = _satisfying_witness(O, field, k, gate_T, fixed, rng)
    zeroE = np.zeros((rows, 4), np.uint64)
    # both are satisfying instances with u = 1, E = 0 (a fresh PlonkInstance viewed as relaxed)
    assert St.is_sat_gates(W1, y1) == 0 and St.is_sat_gates(W2, y2) == 0
    ch1 = np.concatenate([y1.reshape(-1, 4), one.reshape(1, 4)])
    assert St.is_sat_gates(W1, ch1, zeroE) == 0
    ck = S.CommitmentKey.setup_synthetic(curve, nadv * rows, seed=5)
    terms, commits = S.VanillaFS.commit_cross_terms(ck, St, y1, one, W1, y2, W2)
    # Q4: the last cross term (pure W2, u2 = 1) of a satisfied fresh instance is identically zero -> identity commitment
    assert not terms[-1].any() and not commits[-1].any()
    r = rand_fe(rng, 1)[0]
    acc = S.RelaxedPlonkWitness(field, [W1], zeroE).fold([W2], terms, r)
    chf = O.fe_add(field, ch1, O.fe_mul(field, np.broadcast_to(r, ch1.shape).copy(), np.concatenate([y2.reshape(-1, 4), one.reshape(1, 4)])))
    assert St.is_sat_gates(acc.W[0], chf, acc.E) == 0                      # folded accumulator satisfies the relaxed relation
    bad = acc.E.copy(); bad[3] = one
    assert St.is_sat_gates(acc.W[0], chf, bad) == 1
    sf = O.SCALAR_FIELD[curve]
    rp = [r]
    for _ in range(len(terms) - 1):
        rp.append(O.fe_mul(sf, rp[-1].reshape(1, 4), r.reshape(1, 4))[0])
    assert np.array_equal(ck.commit(acc.W[0]), S.point_lincomb(curve, ck.commit(W1), ck.commit(W2).reshape(1, 8), r.reshape(1, 4)))
    assert np.array_equal(ck.commit(acc.E), S.point_lincomb(curve, None, commits, np.stack(rp)))
    # VanillaFS::prove as ONE call (srs_sangria_prove) on device-resident traces: same cross terms, commitments, folds (in place) and
    # folded instance commitments; with an oracle the challenge is squeezed inside from the absorbed commitments
    import torch
    dv = (lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()) if torch.cuda.is_available() else (lambda a: np.ascontiguousarray(a).copy())
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1, 4) if hasattr(t, "cpu") else t
    cW1, cW2 = ck.commit(W1), ck.commit(W2)
    dW1, dE = dv(W1), dv(zeroE)
    pr = S.sangria_prove(ck, St, y1, one, dW1, y2, dv(W2), dE, np.stack([cW1, cW2]), np.zeros(8, np.uint64), r=r)
    assert np.array_equal(pr["commits"], commits) and all(np.array_equal(host(a), b) for a, b in zip(pr["terms"], terms))
    assert np.array_equal(host(dW1), acc.W[0]) and np.array_equal(host(dE), acc.E)
    assert np.array_equal(pr["W_commitment"].wait(), ck.commit(acc.W[0])) and np.array_equal(pr["E_commitment"].wait(), ck.commit(acc.E))
    from oracle import poseidon as OP
    from oracle import pyref as P
    bf = O.BASE_FIELD[curve]
    ro, oro = S.PoseidonHash(bf, 5, 4, 10, 10), OP.PoseidonHash(P.MODULI[bf], 5, 4, 10, 10)
    ro.absorb_point(curve, cW1); oro.absorb_point(tuple(O.mont_to_ints(bf, cW1.reshape(2, 4))))
    dW1b, dEb = dv(W1), dv(zeroE)
    pr2 = S.sangria_prove(ck, St, y1, one, dW1b, y2, dv(W2), dEb, np.stack([cW1, cW2]), np.zeros(8, np.uint64), ro=ro)
    for c in commits:
        oro.absorb_point(tuple(O.mont_to_ints(bf, c.reshape(2, 4))))
    assert O.mont_to_ints(sf, pr2["r"]) == [oro.squeeze(128)]
    assert np.array_equal(host(dW1b), O.fold_w(field, W1, W2, pr2["r"]))
    pr2["W_commitment"].wait(); pr2["E_commitment"].wait()
    # srs_sangria_prove_incoming: the incoming trace arrives from the HOST without a commitment -- uploaded, committed in the same batched
    # MSM as the cross terms, absorbed (+ the rest of U2: `u2_tail`) before the cross-term commitments
    if nch:     # a structure with challenges: U2's challenges come after its commitment (src/plonk/mod.rs:465-495) -> the merged entry refuses
        with pytest.raises(Exception) as ei:
            S.sangria_prove(ck, St, y1, one, dv(W1), y2, dv(W2), dv(zeroE), cW1, np.zeros(8, np.uint64), r=r, incoming=True)
        assert "challenges" in str(ei.value)
        St.close()
        return
    tail = rand_fe(rng, 3)
    ro3, oro3 = S.PoseidonHash(bf, 5, 4, 10, 10), OP.PoseidonHash(P.MODULI[bf], 5, 4, 10, 10)
    ro3.absorb_point(curve, cW1); oro3.absorb_point(tuple(O.mont_to_ints(bf, cW1.reshape(2, 4))))
    dW1c, dEc, dW2c = dv(W1), dv(zeroE), dv(np.zeros_like(W2))
    pr3 = S.sangria_prove(ck, St, y1, one, dW1c, y2, dW2c, dEc, cW1, np.zeros(8, np.uint64), ro=ro3, incoming=True, incoming_host=W2,
                          u2_tail=tail)
    assert np.array_equal(pr3["incoming_commitment"], cW2) and np.array_equal(host(dW2c), W2)
    assert np.array_equal(pr3["commits"], commits) and all(np.array_equal(host(a), b) for a, b in zip(pr3["terms"], terms))
    oro3.absorb_point(tuple(O.mont_to_ints(bf, cW2.reshape(2, 4))))
    oro3.absorb_field_iter(O.mont_to_ints(bf, tail))
    for c in commits:
        oro3.absorb_point(tuple(O.mont_to_ints(bf, c.reshape(2, 4))))
    assert O.mont_to_ints(sf, pr3["r"]) == [oro3.squeeze(128)]
    assert np.array_equal(host(dW1c), O.fold_w(field, W1, W2, pr3["r"])) and np.array_equal(host(dEc), O.fold_e(field, zeroE, terms, pr3["r"]))
    assert np.array_equal(pr3["W_commitment"].wait(), S.point_lincomb(curve, cW1, cW2.reshape(1, 8), pr3["r"].reshape(1, 4)))
    pr3["E_commitment"].wait()
    # ... with a given challenge and a resident trace it equals srs_sangria_prove
    dW1d, dEd = dv(W1), dv(zeroE)
    pr4 = S.sangria_prove(ck, St, y1, one, dW1d, y2, dv(W2), dEd, cW1, np.zeros(8, np.uint64), r=r, incoming=True)
    assert np.array_equal(pr4["incoming_commitment"], cW2) and np.array_equal(host(dW1d), acc.W[0]) and np.array_equal(host(dEd), acc.E)
    assert np.array_equal(pr4["W_commitment"].wait(), ck.commit(acc.W[0])) and np.array_equal(pr4["E_commitment"].wait(), ck.commit(acc.E))
    # a key shorter than the trace: the reference's TooLongInput, before anything is written
    short = S.CommitmentKey.setup_synthetic(curve, rows, seed=5)
    dW1e = dv(W1)
    with pytest.raises(Exception) as ei:
        S.sangria_prove(short, St, y1, one, dW1e, y2, dv(W2), dv(zeroE), cW1, np.zeros(8, np.uint64), r=r, incoming=True)
    assert "too long input" in str(ei.value) and np.array_equal(host(dW1e), W1)
    short.close()
    St.close()


def test_fold_then_decider(srs, oracle):
    _fold_then_decide(srs, oracle, 0, 0, 7, (5, 3))     # primary: bn256 / Fr, 2 gates (challenge y folds too)
    _fold_then_decide(srs, oracle, 1, 1, 6, (5,))       # secondary: grumpkin / Fq


def _high_degree_gates(M, n_gates):
    """n gates q_i * (a * b(rot) - c) over n fixed and 3 advice columns, in oracle.expr's (M.Poly) or sirius_amd.expression's spelling"""
    nfix = n_gates
    mk = lambda i: M.Prod(M.Poly(i), M.Sum(M.Prod(M.Poly(nfix), M.Poly(nfix + 1, 1 if i % 3 == 0 else 0)), M.Neg(M.Poly(nfix + 2)))) \
        if hasattr(M, "Poly") else M.Product(M.Polynomial(i), M.Sum(M.Product(M.Polynomial(nfix), M.Polynomial(nfix + 1, 1 if i % 3 == 0 else 0)), M.Negated(M.Polynomial(nfix + 2))))
    return [mk(i) for i in range(n_gates)]


def _high_degree_case(S, O, field, k, n_gates):
    """Folding degree above 8 (n gates compressed with y^(n-1): degree = 2 + n - 1): the cross terms take several
    passes over the evaluation points, the error fold several launches.  Checked against the reference's symbolic
    GroupedPoly route and through fold-then-decide."""
    from workloads import rand_fe
    X = S.expression
    rows = 1 << k
    rng = np.random.default_rng(n_gates * 7 + k)
    nfix, nadv = n_gates, 3
    og = _high_degree_gates(OE, n_gates)
    pg = _high_degree_gates(X, n_gates)
    fixed = [rand_fe(rng, rows, 0.5) for _ in range(nfix)]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    St = S.PlonkStructure(field, k, [], fixed, nadv, pg)
    assert St.num_cross_terms == n_gates + 1 and St.num_challenges == 1
    u1c, u1u, u2c = rand_fe(rng, 1), rand_fe(rng, 1)[0], rand_fe(rng, 1)
    terms, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, W1, u2c, W2)
    ch = S.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    cg, exp = OE.cross_terms_oracle(O, field, og, 0, nfix, nadv, [], fixed, W1, W2, ch)
    assert len(terms) == cg.degree == n_gates + 1
    for a, b in zip(terms, exp):
        assert np.array_equal(a, b)
    r, E = rand_fe(rng, 1)[0], rand_fe(rng, rows)
    acc = S.RelaxedPlonkWitness(field, [W1], E).fold([W2], terms, r)
    assert np.array_equal(acc.E, O.fold_e(field, E, exp, r))
    # definition of the cross terms: P_hom(fold) == P_hom(W1) + sum r^k T_k
    one = O.ints_to_mont(field, [1])[0]
    ch1 = np.concatenate([u1c.reshape(-1, 4), u1u.reshape(1, 4)])
    ch2 = np.concatenate([u2c.reshape(-1, 4), one.reshape(1, 4)])
    chf = O.fe_add(field, ch1, O.fe_mul(field, np.broadcast_to(r, ch2.shape).copy(), ch2))
    p0 = St.eval_gates(W1, ch1, homogeneous=True)
    rhs = S.RelaxedPlonkWitness(field, [], p0).fold([], terms, r).E
    assert St.is_sat_gates(acc.W[0], chf, rhs) == 0
    St.close()


def test_high_folding_degree(srs, oracle):
    _high_degree_case(srs, oracle, 0, 6, 10)      # degree 11: two passes
    _high_degree_case(srs, oracle, 1, 8, 14)      # degree 15
    # (the symbolic oracle grows exponentially with the gate count; 17+ gates = three passes run in the emulator-free
    #  property test below)
    _high_degree_props(srs, oracle, 0, 10, 30)


def _high_degree_props(S, O, field, k, n_gates):
    """degree 31 (four passes) without the symbolic oracle: the defining identity of the cross terms."""
    from workloads import rand_fe
    X = S.expression
    rows = 1 << k
    rng = np.random.default_rng(n_gates)
    nfix, nadv = n_gates, 3
    pg = [X.Product(X.Polynomial(i), X.Sum(X.Product(X.Polynomial(nfix), X.Polynomial(nfix + 1)), X.Negated(X.Polynomial(nfix + 2))))
          for i in range(n_gates)]
    fixed = [rand_fe(rng, rows, 0.5) for _ in range(nfix)]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    St = S.PlonkStructure(field, k, [], fixed, nadv, pg)
    assert St.num_cross_terms == n_gates + 1
    u1c, u1u, u2c = rand_fe(rng, 1), rand_fe(rng, 1)[0], rand_fe(rng, 1)
    terms, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, W1, u2c, W2)
    one = O.ints_to_mont(field, [1])[0]
    ch1 = np.concatenate([u1c.reshape(-1, 4), u1u.reshape(1, 4)])
    ch2 = np.concatenate([u2c.reshape(-1, 4), one.reshape(1, 4)])
    for _ in range(2):
        r = rand_fe(rng, 1)[0]
        acc = S.RelaxedPlonkWitness(field, [W1], St.eval_gates(W1, ch1, homogeneous=True)).fold([W2], terms, r)
        chf = O.fe_add(field, ch1, O.fe_mul(field, np.broadcast_to(r, ch2.shape).copy(), ch2))
        assert St.is_sat_gates(acc.W[0], chf, acc.E) == 0
    # the last term is P_hom(W2, ch2) itself (coefficient of X^d)
    assert np.array_equal(terms[-1], St.eval_gates(W2, ch2, homogeneous=True))
    St.close()


def _row_shard_case(S, O, field, curve, k, gate_T, world=2, with_commit=True):
    """Multi-GPU row sharding (srs_structure_set_shard): every rank evaluates the cross terms on the rows of its own
    block-cyclic stripes only; together with the sharded key the partial commitments still add up to commit(T_k)."""
    from workloads import rand_fe
    gate_T = list(gate_T)
    rows = 1 << k
    gates, nfix, nadv = gates_for(gate_T)
    rng = np.random.default_rng(k + world)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    nch = St.num_challenges
    u1c, u1u, u2c = rand_fe(rng, nch), rand_fe(rng, 1)[0], rand_fe(rng, nch)
    full, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, W1, u2c, W2)
    ch = S.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    _, exp = OE.cross_terms_oracle(O, field, _oracle_gates(gate_T), 0, nfix, nadv, [], fixed, W1, W2, ch)
    for a, b in zip(full, exp):
        assert np.array_equal(a, b)
    bases = O.make_bases(curve, 9, rows) if with_commit else None
    ck_full = S.CommitmentKey(curve, bases) if with_commit else None
    want = np.stack([ck_full.commit(t) for t in full]) if with_commit else None
    stripe = np.arange(rows) >> 10
    partials = []
    for rank in range(world):
        St.set_shard(rank, world)
        ck = S.CommitmentKey(curve, bases, rank=rank, world=world) if with_commit else None
        terms, commits = S.VanillaFS.commit_cross_terms(ck, St, u1c, u1u, W1, u2c, W2)
        mine = (stripe % world) == rank
        for t, e in zip(terms, exp):
            assert np.array_equal(t[mine], e[mine])              # local stripes: the reference's values
            assert not t[~mine].any()                            # (freshly zeroed buffers) the other stripes were not written
        partials.append(commits)
        if ck is not None:
            ck.close()
    St.set_shard(0, 1)
    again, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, W1, u2c, W2)       # unsharded again: every row
    assert all(np.array_equal(a, b) for a, b in zip(again, exp))
    if with_commit:
        for j in range(len(full)):
            assert np.array_equal(S.point_sum(curve, np.stack([p[j] for p in partials])), want[j])
        ck_full.close()
    St.close()


def test_row_sharded_cross_terms(srs, oracle):
    _row_shard_case(srs, oracle, 0, 0, 13, (5, 3), 2)       # ahead-of-time kernel
    _row_shard_case(srs, oracle, 1, 1, 12, (3, 2), 3)       # interpreter, world not a power of two
    _row_shard_case(srs, oracle, 1, 1, 14, (2, 2), 4)       # run-time compiled kernel


def test_non_contiguous_and_int64_inputs(srs, oracle):
    """ADVICE r01 / r02 regression: strided views and int64-typed host arrays through RelaxedPlonkWitness.fold, lookup_coeff_2 and
    batch_invert_assigned -- the converted temporaries must outlive the C call (tests/input_forms_cases.py)."""
    from input_forms_cases import run_input_forms_case
    run_input_forms_case(srs, oracle, 0, 3000, 12)
    run_input_forms_case(srs, oracle, 1, 1000, 4)
