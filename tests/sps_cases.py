"""Trace-generation cases shared by the GPU parity tests and the CPU emulator tests: srs_run_sps_protocol
(PlonkStructure::run_sps_protocol, src/plonk/mod.rs:413-662) as ONE call against the literal protocol composed from oracle parts --
oracle.lookup.evaluate_coefficient_1 / _2 for the lookup rounds, oracle.msm on the key's bases for every commitment and
oracle.poseidon.PoseidonHash (T = 5, RATE = 4, R_F = 10, R_P = 10 over the curve's base field) for the transcript: instances
(reduced modulo the oracle field's modulus, util::fe_to_fe), then absorb_point(C_i) and squeeze(128) after every round.  The product
must equal it in every round vector, every commitment and every challenge, bit for bit.

Circuits: the lookup variants of tests/lookup_cases.py ("vector" -> _3, "scalar" -> _2, "two" -> _2 with two lookups: the grouped
ls | ts | ms and hs | gs layout and the per-lookup launches) and two shapes without lookups ("one": one gate -> _0, "gates": two
gates -> _1).  The device vector the call fills starts out as a byte pattern: padding must be WRITTEN as zeros.
"""
import ctypes as C

import numpy as np

from lookup_cases import _circuit, _shape, _sps_product, _to_product_expr
from oracle import expr as OE
from oracle import lookup as OL
from oracle import pyref as P
from oracle.poseidon import PoseidonHash as OraclePoseidon

RO_PARAMS = (5, 4, 10, 10)          # T, RATE, R_F, R_P
PATTERN = 0xAB


def _plain_shape(variant):
    """no lookups: "one" = one gate (no challenge), "gates" = two gates (the compression challenge)"""
    ns, nf, na = 2, 1, 3
    s_add, s_mul, f = OE.Poly(0), OE.Poly(1), OE.Poly(2)
    a, b, c = [OE.Poly(ns + nf + i) for i in range(3)]
    gates = [OE.Prod(s_add, OE.Sum(OE.Sum(a, b), OE.Neg(c)))]
    if variant == "gates":
        gates.append(OE.Prod(s_mul, OE.Sum(OE.Prod(a, b), OE.Neg(OE.Prod(f, c)))))
    return ns, nf, na, gates, []


def _fe(O, field, rng, n):
    return O.ints_to_mont(field, [int(rng.integers(0, 1 << 62)) * int(rng.integers(1, 1 << 62)) + 1 for _ in range(n)])


class Circuit:
    def __init__(self, S, O, curve, variant, k, seed=0):
        X = S.expression
        self.curve, self.variant, self.k, self.rows = curve, variant, k, 1 << k
        self.field = field = O.SCALAR_FIELD[curve]
        self.rng = rng = np.random.default_rng(3000 + 17 * k + len(variant) + seed)
        if variant in ("one", "gates"):
            ns, nf, na, ogates, olookups = _plain_shape(variant)
            self.selectors = [rng.integers(0, 2, size=self.rows).astype(np.uint8) for _ in range(ns)]
            self.fixed = [_fe(O, field, rng, self.rows) for _ in range(nf)]
            self.advice = lambda: [_fe(O, field, rng, self.rows) for _ in range(na)]
        else:
            ns, nf, na, ogates, olookups = _shape(variant)
            self.selectors, self.fixed, self.advice = _circuit(O, field, variant, k, rng)
        self.na = na
        self.meta = OL.build_metainfo(k, ns, nf, na, ogates, olookups)
        self.St = S.PlonkStructure(field, k, self.selectors, self.fixed, na, [_to_product_expr(X, g) for g in ogates],
                                   lookups=[([_to_product_expr(X, e) for e in i], [_to_product_expr(X, e) for e in t]) for i, t in olookups] or None)
        St, meta = self.St, self.meta
        assert St.num_challenges == meta.num_challenges and St.num_rounds == len(meta.round_sizes)
        assert [St.round_len(i) for i in range(St.num_rounds)] == meta.round_sizes == St.round_sizes and St.round_len(St.num_rounds) == 0

    def close(self):
        self.St.close()


def expected_trace(O, c, cols, instances_int, bases, supplied=None):
    """the literal run_sps_protocol_0 .. _3 -> (rounds, commitments, challenges as ints); supplied: the challenges when no oracle runs"""
    meta, curve, field = c.meta, c.curve, c.field
    bfield = O.BASE_FIELD[curve]
    p, bp = P.MODULI[field], P.MODULI[bfield]
    ro = OraclePoseidon(bp, *RO_PARAMS)
    rounds, cms, chs = [], [], []

    def close_round(W):
        Cm = O.msm(curve, W, bases[:len(W)])
        rounds.append(W)
        cms.append(Cm)
        if len(chs) < meta.num_challenges:
            if supplied is not None:
                chs.append(supplied[len(chs)])
            else:
                chs.append(ro.absorb_point(tuple(O.mont_to_ints(bfield, Cm.reshape(2, 4)))).squeeze(128))
    full = [np.concatenate([col, np.zeros((c.rows - len(col), 4), np.uint64)]) for col in cols]      # concatenate_with_padding
    if meta.num_challenges:
        ro.absorb_field_iter(v % bp for v in instances_int)          # fe_to_fe: reduced modulo the oracle field's modulus
    if meta.num_lookups == 0:
        close_round(OL._concat(full))
    elif not meta.has_vector_lookup:
        c1 = OL.evaluate_coefficient_1(O, field, meta.arguments, c.selectors, c.fixed, full, 0, p)
        close_round(OL._concat(full + c1.ls + c1.ts + c1.ms))
        hs, gs = OL.evaluate_coefficient_2(O, field, c1, chs[0], p)
        close_round(OL._concat(hs + gs))
    else:
        close_round(OL._concat(full))
        c1 = OL.evaluate_coefficient_1(O, field, meta.arguments, c.selectors, c.fixed, full, chs[0], p)
        close_round(OL._concat(c1.ls + c1.ts + c1.ms))
        hs, gs = OL.evaluate_coefficient_2(O, field, c1, chs[1], p)
        close_round(OL._concat(hs + gs))
    return rounds, cms, chs


def fresh_W(sp, c):
    return sp.dev(np.full((c.St.num_witness_columns * c.rows, 4), PATTERN * 0x0101010101010101, dtype=np.uint64))


def product_oracle(S, c):
    return S.PoseidonHash(1 - c.field, *RO_PARAMS)        # the base field of the curve whose scalar field is c.field


def run_case(S, O, sp, key, curve, variant, k, space="host", lens=None, instances_int=(3, 1 << 200, 0), supplied=None, stepwise=True,
             witness_commit=True, decide=True, cols=None, circuit=None):
    """one trace through the one call, compared with the literal protocol; -> (circuit, result, expected) for further checks"""
    ck, bases = key
    c = circuit or Circuit(S, O, curve, variant, k)
    St, field = c.St, c.field
    cols = cols if cols is not None else c.advice()
    if lens is not None:
        cols = [np.ascontiguousarray(col[:n]) for col, n in zip(cols, lens)]
    inst = O.ints_to_mont(field, list(instances_int))
    rounds, cms, chs = expected_trace(O, c, cols, instances_int, bases, supplied)
    ro = None if supplied is not None else product_oracle(S, c)
    out = St.run_sps_protocol(ck, inst, [sp.dev(col) for col in cols] if space == "dev" else cols, ro=ro,
                              challenges=None if supplied is None else O.ints_to_mont(field, list(supplied)), W=fresh_W(sp, c))
    what = (curve, variant, k, space)
    assert len(out["rounds"]) == len(rounds) == St.num_rounds
    for i, (a, b) in enumerate(zip(out["rounds"], rounds)):
        assert np.array_equal(sp.host(a), b), (what, "round", i)
    assert np.array_equal(out["W_commitments"], np.array(cms)), (what, "commitments")
    want_ch = O.ints_to_mont(field, chs) if chs else np.zeros((0, 4), np.uint64)
    assert np.array_equal(out["challenges"], want_ch), (what, "challenges")
    if ro is not None and chs:          # the oracle is left where the reference leaves it: the next squeeze agrees
        bfield = O.BASE_FIELD[curve]
        again = OraclePoseidon(P.MODULI[bfield], *RO_PARAMS)
        again.absorb_field_iter(v % P.MODULI[bfield] for v in instances_int)
        for Cm in cms[:len(chs)]:
            again.absorb_point(tuple(O.mont_to_ints(bfield, Cm.reshape(2, 4))))
        assert O.mont_to_ints(field, ro.squeeze(128, field))[0] == again.squeeze(128), (what, "oracle state")
    if c.meta.num_lookups and stepwise:      # the step-wise calls the one call replaces, under the same challenges
        step = _sps_product(S, St, cols, out["challenges"])
        for i, (a, b) in enumerate(zip(out["rounds"], step)):
            assert np.array_equal(sp.host(a), b), (what, "step-wise round", i)
    if witness_commit:
        assert S.VanillaFS.is_sat_witness_commit(ck, out["rounds"], out["W_commitments"]) == (0, False), what
    if c.meta.num_lookups == 1 and decide:    # the satisfiable variants: the deciders accept the returned vector as it stands
        assert St.is_sat_gates(out["W"], out["challenges"]) == 0 and St.is_sat_log_derivative(out["W"]) == 0, what
    if circuit is None:
        c.close()
    return c, out, (rounds, cms, chs)


def zero_denominator_case(S, O, sp, key, curve=0, k=6):
    """ro = NULL, "scalar": r1 = -l[j] for a looked-up row j, then r1 = -t[i] for a table row i: 1/0 lands as 0 in h and g"""
    c = Circuit(S, O, curve, "scalar", k)
    p = P.MODULI[c.field]
    cols = c.advice()
    q = c.rows // 4
    j, i = q + 1, 5                                            # a row the selector looks up; the table row holding 5
    l_j = O.mont_to_ints(c.field, cols[0][j:j + 1])[0]         # l = s_rc * a
    t_i = O.mont_to_ints(c.field, c.fixed[0][i:i + 1])[0]
    assert c.selectors[1][j] == 1 and l_j < 8 and t_i == 5
    for r1, col, row in (((p - l_j) % p, 0, j), ((p - t_i) % p, 1, i)):
        _, out, (rounds, _, _) = run_case(S, O, sp, key, curve, "scalar", k, supplied=[r1, 0x1234567], cols=cols, circuit=c,
                                          witness_commit=False, decide=False)       # (the gate h (l + r) = 1 cannot hold on a zero denominator)
        hg = rounds[1].reshape(2, c.rows, 4)                   # hs | gs
        assert not hg[col][row].any(), ("the oracle has no zero at the chosen row", col, row)
        assert not sp.host(out["rounds"][1]).reshape(2, c.rows, 4)[col][row].any()
    c.close()


def _raw(S, St, ck, ro, inst, cols, lens, W_addr, ch, cm):
    L = S._lib
    ptrs = (C.c_void_p * max(len(cols), 1))(*[col.ctypes.data for col in cols])
    ln = (C.c_size_t * max(len(cols), 1))(*lens)
    return L.lib().srs_run_sps_protocol(St._h, ck._h, None if ro is None else ro._h, inst.ctypes.data, inst.shape[0], ptrs, ln, len(cols),
                                        L.SPACE_HOST, W_addr, None, ch.ctypes.data, cm.ctypes.data)


def refusal_cases(S, O, sp, key, curve=0):
    """every refusal comes before anything is written: commitments, challenges, the device vector and the oracle stay as they were"""
    L = S._lib
    ck, bases = key
    sc = Circuit(S, O, curve, "scalar", 6)                     # round 0 = 6 * 2^6
    pl = Circuit(S, O, curve, "gates", 5)
    small = S.CommitmentKey(curve, bases[:1 << 8])
    sharded = S.CommitmentKey(curve, bases[:1 << 10], rank=0, world=2)
    wrong_ro = S.PoseidonHash(sc.field, *RO_PARAMS)            # over the SCALAR field
    inst = O.ints_to_mont(sc.field, [7, 8])

    def refused(c, k, ro, cols, lens, rc, text):
        ro = ro or product_oracle(S, c)
        ro.absorb_field(O.ints_to_mont(ro.field, [99]))
        before = ro.squeeze(128, c.field)
        W = fresh_W(sp, c)
        ch = np.full((3, 4), 0x5A5A5A5A5A5A5A5A, np.uint64)
        cm = np.full((3, 8), 0xC3C3C3C3C3C3C3C3, np.uint64)
        got = _raw(S, c.St, k, ro, inst, cols, lens, sp.addr(W), ch, cm)
        assert got == rc, (text, got, L.lib().srs_last_error())
        assert text in L.lib().srs_last_error().decode(), (text, L.lib().srs_last_error())
        assert (ch == 0x5A5A5A5A5A5A5A5A).all() and (cm == 0xC3C3C3C3C3C3C3C3).all(), text
        assert (sp.host(W).view(np.uint8) == PATTERN).all(), text
        assert np.array_equal(ro.squeeze(128, c.field), before), text

    cols = sc.advice()
    full = [sc.rows] * 3
    refused(sc, small, None, cols, full, L.ERR_TOO_LONG_INPUT, "too long input")
    refused(sc, ck, None, cols[:2], full[:2], L.ERR_INVALID, "2 columns for 3 advice columns")
    refused(sc, ck, None, cols, [sc.rows, sc.rows - 3, sc.rows], L.ERR_INVALID, "shorter than 2^k")
    refused(sc, ck, wrong_ro, cols, full, L.ERR_INVALID, "base field")
    refused(sc, sharded, None, cols, full, L.ERR_INVALID, "sharded")
    pcols = pl.advice()
    long_col = np.concatenate([pcols[1], pcols[1][:1]])
    refused(pl, ck, None, [pcols[0], long_col, pcols[2]], [pl.rows, pl.rows + 1, pl.rows], L.ERR_INVALID, "longer than 2^k")
    for h in (small, sharded):
        h.close()
    sc.close()
    pl.close()
