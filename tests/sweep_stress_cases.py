"""Stress gates and adversarial inputs for the sweep form of the row programs (csrc/rowprog_compile.hip, emit_sweep_source), shared by
the bound audit on the emulator (tests/test_sweep_bounds_emu.py) and the GPU parity tests (tests/test_sweep_bounds_gpu.py).

The emitter keeps a static bound "in units of p" for every lazy value and inserts a reducing product where a threshold is passed.
Which contract of csrc/field29.cuh each threshold serves (R = 2^261 / p, 169.2 for Fr and Fq):
  12   an operand of a product: mul needs A * B < R p^2, and 12 * 12 = 144 < R
  30   an operand of a lazy add / sub: the sum is <= 61 p, a subtraction's CP <= 31 (kp() is stated for c <= 64), and after the
       normalize the value still fits nine 29-bit limbs (< R p)
  12   a group of same-coefficient terms: its closing product with the canonical coefficient is 12 * 1 < R
  24   the cluster total, and 100, the LDS accumulator: 100 + 24 (+ 2 handed in) < R, so the accumulator always fits nine limbs and
       its folding product with 2^261 mod p (canonical) is < R p^2
  2 (1 + points) for a hoisted affine factor: with at most DMAX + 1 = 9 points it is used at <= 18 p, so its partner is prepared to
       <= 8 p (18 * 8 = 144 < R; the emitter budgets 20 p * 8 p)
  vb + sb * DMAX for an affine cluster: the value at the last of <= DMAX + 1 points
Every gate below is built so that ONE of these branches is taken; `marks` are the substrings of the emitted source
(srs_structure_program_source) that show it, `which` the program they are looked for in (0 cross terms, 1 compressed).

Gates are the node tuples sirius_amd.expression and oracle.expr share.  Inputs are Montgomery WORDS chosen from WORDS(field): any
4 x u64 word below p is a valid element, and tests/workloads.rand_fe only ever produces words below 2^253 -- a third of Fr, every
word with the top limb of the 9 x 29-bit form above 2^21, never met a row program before."""
import functools

import numpy as np

from oracle import pyref as P

ROWS = 64            # the pattern's period; 2^14-row inputs of the run-time compiled kernels are this pattern tiled
BLOCK = 4            # rows per extreme block: with rotations 0..3 row 0 of a block sees only that block's word


def word_ints(field):
    """the chosen words, as integers: 0, 1, 2, p-1, p-2, (p-1)/2, (p+1)/2, 2^253-1, 2^253, 2^232-1 (eight saturated 29-bit limbs)
    and one seeded uniform word below p"""
    p = P.MODULI[field]
    import random
    return [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, (1 << 253) - 1, 1 << 253, (1 << 232) - 1, random.Random(29 + field).randrange(p)]


@functools.lru_cache(maxsize=None)
def words(field):
    """(11, 4) uint64: word_ints as little-endian 4 x u64 words"""
    w = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in word_ints(field)], dtype=np.uint64)
    w.setflags(write=False)
    return w


def column(field, seed, rows=ROWS):
    """(rows, 4): rows 0..3 all p-1, rows 4..7 all 2^253-1, rows 8..11 all 0 (so that, for every gate, one row has EVERY operand at
    p-1, one at 2^253-1 and one at 0, rotations included), the rest a seeded mix of the whole set; period ROWS"""
    W = words(field)
    idx = np.random.default_rng(seed).integers(0, W.shape[0], size=ROWS)
    idx[0:BLOCK], idx[BLOCK:2 * BLOCK], idx[2 * BLOCK:3 * BLOCK] = 3, 7, 0
    col = W[idx]
    assert rows % ROWS == 0
    return np.ascontiguousarray(np.tile(col, (rows // ROWS, 1)))


def columns(field, n, seed, rows=ROWS):
    """n columns stacked column-major: (n * rows, 4)"""
    return np.ascontiguousarray(np.concatenate([column(field, seed * 1000 + i, rows) for i in range(n)])) if n else np.zeros((0, 4), np.uint64)


def picks(field, n, seed):
    """(n, 4): n seeded picks of the set (challenges, u, betas, delta)"""
    W = words(field)
    return np.ascontiguousarray(W[np.random.default_rng(seed).integers(0, W.shape[0], size=n)]).reshape(n, 4)


def inputs(field, nsel, nfix, nadv, seed, rows=ROWS):
    """selectors, fixed columns, W1, W2 of one case, all from the set"""
    rng = np.random.default_rng(seed)
    sels = [np.tile((rng.random(ROWS) < 0.7).astype(np.uint8), rows // ROWS) for _ in range(nsel)]
    fixed = [column(field, seed * 1000 + 500 + i, rows) for i in range(nfix)]
    return sels, fixed, columns(field, nadv, 2 * seed + 1, rows), columns(field, nadv, 2 * seed + 2, rows)


# ---------------------------------------------------------------------------------------------------------------- the gates
def _sum(xs):
    """a balanced tree of sums (the compiler distributes the linear skeleton down to depth 64 only: see deep_sum)"""
    return xs[0] if len(xs) == 1 else ('sum', _sum(xs[:len(xs) // 2]), _sum(xs[len(xs) // 2:]))


def _chain(xs):
    """a left-nested chain of sums: depth len(xs) - 1"""
    acc = xs[0]
    for x in xs[1:]:
        acc = ('sum', acc, x)
    return acc


def _pow(x, e):
    """x^e by squarings (e a power of two) or a left-nested chain"""
    if e & (e - 1) == 0:
        while e > 1:
            x, e = ('prod', x, x), e // 2
        return x
    acc = x
    for _ in range(e - 1):
        acc = ('prod', acc, x)
    return acc


class Case:
    """name, field, columns, the gate; what the emitted sweep source of program `which` must show: `marks` (substrings), the number of
    `clusters`, at least `folds` reducing products with 2^261 mod p (U[<one>]) and exactly `acc_folds` foldings of the LDS accumulator;
    `degree`: the folding degree (as many cross terms, degree + 1 points); jit: the run-time compiler takes it (degree <= 8)"""

    def __init__(self, name, field, nfix, nadv, gate, marks, which=0, degree=None, jit=True, clusters=None, folds=0, acc_folds=0):
        self.name, self.field, self.nsel, self.nfix, self.nadv, self.gates = name, field, 0, nfix, nadv, [gate]
        self.marks, self.which, self.degree, self.jit = marks, which, degree, jit
        self.clusters, self.folds, self.acc_folds = clusters, folds, acc_folds

    def __repr__(self):
        return self.name


def _hoist(m, field):
    """q * (s * (a_1 + ... + a_m)) + a_1^8: the hoisted factor q s grows by its step once per point, 2p (1 + point) -- 18p at the ninth
    point, which the folding degree 8 of the second term reaches -- and meets the partner a_1 + ... + a_m, whose bound is m"""
    F = lambda i: ('poly', i, 0)
    A = lambda j, r=0: ('poly', 1 + j, r)
    g = ('sum', ('prod', F(0), ('prod', A(0), _sum([A(1 + i) for i in range(m)]))), _pow(A(1), 8))
    return Case(f"hoist_{m}", field, 1, m + 1, g, ["f29_t aff"], degree=8, folds=1 if m > 8 else 0)


def _pairs(nfix, nadv, n):
    """n distinct terms (f_i a_j) a_k over nfix fixed and nadv advice columns: one level and one degree, hence one coefficient, and
    written so that no factor q (s y) is hoisted"""
    F = lambda i: ('poly', i, 0)
    A = lambda j: ('poly', nfix + j, 0)
    out = []
    for i in range(nfix):
        for j in range(nadv):
            for k in range(nadv):
                out.append(('prod', ('prod', F(i), A(j)), A(k)))
    assert len(out) >= n
    return out[:n]


def cases():
    """the stress gates: (Case, ...) -- built once, read only"""
    return _cases()


@functools.lru_cache(maxsize=None)
def _cases():
    F = lambda i: ('poly', i, 0)
    out = []
    # hoisted factors, partner bound 2 (fits as it is), 9 / 10 / 12 (above 8: folded before it meets the factor)
    for m, field in ((2, 1), (9, 0), (10, 0), (12, 1)):
        out.append(_hoist(m, field))
    # 90 terms of one coefficient in one cluster: the group passes 12 fifteen times; unfolded it would reach 180 > R
    # (six fixed + four advice columns are exactly the 112 registers a cluster may spend on columns)
    out.append(Case("group_90", 0, 6, 4, _sum(_pairs(6, 4, 90)), [], degree=2, clusters=1, folds=14))
    # 90 coefficient groups in one cluster: the total passes 24 seven times; unfolded it would reach 180 > R
    out.append(Case("total_90", 1, 6, 4, _sum([('scaled', t, 3 + i) for i, t in enumerate(_pairs(6, 4, 90))]), [], degree=2, clusters=1, folds=7))
    # ten clusters of eight SUBTRACTED coefficient groups (a group < 2p is subtracted with CP = 3): every cluster adds 24, so the accumulator passes 100 at the fifth cluster and again at
    # the tenth.  A cluster is one product (f_0 a) (f_1 + .. + f_10) over one advice column and eleven fixed columns of its own -- 104 of
    # the 112 budgeted registers, so the next cluster's columns do not fit -- scaled by eight constants (the body is computed once)
    terms = []
    for c in range(10):
        f = lambda i: ('poly', 11 * c + i, 0)
        t = ('prod', ('prod', f(0), ('poly', 110 + c, 0)), _chain([f(i) for i in range(1, 11)]))
        terms += [('neg', ('scaled', t, 3 + j)) for j in range(8)]
    out.append(Case("accumulator_240", 0, 110, 10, _sum(terms), [], degree=1, clusters=10, acc_folds=2))
    # subtraction and negation chains inside a product: CP 21 and 23, a difference of bound 46 (> 30: folded before the next sum),
    # and the sum of bound 22 as a multiplier operand (> 12: folded)
    A = lambda j, r=0: ('poly', 1 + j, r)
    # (the compiler has no subtraction node: a - b is a + (-b), so inside a product only neg_lazy appears; between the TERMS of a
    # group and the groups of a cluster a negative sign is a sub_lazy)
    # (the twenty leaves are six loads, repeated: an advice load is what costs the run-time compiler its time)
    s1 = _chain([A(j % 3, (j // 3) % 2) for j in range(20)])
    s2 = ('sum', A(0), ('neg', s1))
    s3 = ('neg', s2)
    s4 = ('sum', s3, ('neg', s2))
    s5 = ('sum', s4, s1)
    g = ('sum', ('prod', ('prod', F(0), s5), A(1)), ('neg', ('sum', ('prod', A(0), A(1)), ('scaled', ('prod', A(1), A(2)), 9))))
    g = ('sum', ('neg', ('prod', A(2), A(3))), g)
    out.append(Case("sub_chain", 1, 1, 4, g, ["neg_lazy<21, 0>", "neg_lazy<23, 0>", "sub_lazy<3, 0>"], degree=2, folds=2))
    # both operands of a product just above 12: sums of 13 and of 14 column values (13 * 14 = 182 > R unless they are folded)
    out.append(Case("operands_13_14", 0, 1, 3, ('sum', ('prod', _chain([A(j % 3, (j // 3) % 2) for j in range(13)]),
                                                          _chain([A((j + 1) % 3, (j // 3) % 2) for j in range(14)])), ('prod', F(0), A(0))),
                    [], degree=2, folds=2))
    # a left-nested sum of 80 products: below depth 64 the compiler stops distributing, and the 16 deepest products reach the
    # sweep form as ONE term that is a nested sum (bound 32: folded as an operand of the next addition and of the closing product)
    out.append(Case("deep_sum", 0, 6, 4, _chain(_pairs(6, 4, 80)), [], degree=2, clusters=1, folds=1))
    # doubling chain inside a product: 2, 4, .., 32 > 30
    A = lambda j, r=0: ('poly', 1 + j, r)
    d = ('sum', A(0), A(1))
    for _ in range(5):                # the compiler keeps x + x an addition
        d = ('sum', d, d)
    out.append(Case("doubling", 0, 1, 2, ('prod', ('prod', F(0), d), A(1)), [], degree=2, folds=1))
    # constants inside products: a uniform operand of a body addition at level > 0, and a level-0 column raised to level 1
    c = ('prod', ('sum', A(0), ('const', 5)), ('prod', A(1), ('sum', ('sum', ('prod', A(0), A(1)), ('const', 7)), A(2))))
    out.append(Case("const_in_product", 1, 1, 3, ('sum', c, ('prod', F(0), A(0))), [], degree=4))
    # rotations on the hoisted leaf and its partner
    out.append(Case("hoist_rotated", 0, 1, 2, ('sum', ('prod', F(0), ('prod', A(0, 1), ('sum', A(1), A(1, 1)))), ('prod', A(0), A(1, 2))), ["f29_t aff", "(row + 1u) & mask", "(row + 2u) & mask"], degree=2))
    # linear terms next to a product: in the compressed program (no challenge) they form an affine cluster with a non-zero step
    B = lambda j, r=0: ('poly', 3 + j, r)
    out.append(Case("affine", 0, 3, 2, ('sum', ('sum', ('sum', ('prod', F(0), B(0)), ('prod', F(1), B(1, 1))), F(2)), ('prod', B(0), B(1))),
                    ["affine in the point", "cur = G::normalize(G::add_lazy(cur, "], which=1, degree=2, clusters=2, folds=1))
    # folding degree 9: ten points, one more than the sweep form takes
    out.append(Case("degree_9", 1, 1, 2, ('sum', ('prod', F(0), _pow(A(0), 9)), ('prod', A(0), A(1))), [], degree=9, jit=False))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------- running them
def tuples(e):
    """a gate read from JSON (nested lists) as the nested tuples the oracle hashes"""
    return tuple(tuples(x) for x in e) if isinstance(e, (list, tuple)) else e


def program_source(St, which):
    """(emitted source of program `which`, ahead-of-time kernel id or -1 / -2) from srs_structure_program_source"""
    import ctypes as C
    from sirius_amd import _lib
    lib = _lib.lib()
    sid = C.c_int()
    n = lib.srs_structure_program_source(St._h, which, None, 0, None, C.byref(sid))
    buf = C.create_string_buffer(n + 1)
    assert lib.srs_structure_program_source(St._h, which, buf, n + 1, None, None) == n
    return buf.raw[:n].decode(), sid.value


def sweep_part(src):
    """the sweep form of an emitted source (empty: the program has none) and the uniform index of 2^261 mod p in it"""
    import re
    i = src.find("template <class F> __device__ constexpr uint32_t spec_fn_sweep_one()")
    if i < 0:
        return "", None
    return src[i:], int(re.search(r"spec_fn_sweep_one\(\) \{ return (\d+)u; \}", src).group(1))


def check_marks(case, St):
    """the bookkeeping branch the gate was built for is in the emitted program"""
    sw, one = sweep_part(program_source(St, case.which)[0])
    assert sw, (case.name, "no sweep form")
    for m in case.marks:
        assert m in sw, (case.name, "missing in the emitted sweep form", m)
    if case.clusters is not None:
        assert sw.count("{   // cluster ") == case.clusters, (case.name, "clusters", sw.count("{   // cluster "))
    acc_folds = sw.count("sw_store(acc, pt, G::mul(sw_load(acc, pt), G::unpack(U[%d])));" % one)
    folds = sw.count(", G::unpack(U[%d]));" % one)              # products with the radix' one that are not accumulator folds
    assert acc_folds == case.acc_folds, (case.name, "accumulator folds", acc_folds)
    assert folds >= case.folds and (case.folds > 0 or folds == 0), (case.name, "reducing products", folds)


def cross_case(S, O, field, k, nsel, nfix, nadv, gates, seed, tile=1, kinds=(-2, -1)):
    """Cross terms of `gates` on word-set inputs, through the structure as created (kernel kind kinds[0]) and, when kinds[1] is not None,
    under no_jit=1 (kind kinds[1]), against cross_terms_oracle.  The oracle runs on the 2^k-row pattern; the product on the pattern tiled
    `tile` times (rotations wrap modulo a multiple of the period, so the expected output is the oracle's, tiled)."""
    import ctypes as C
    from oracle import expr as OE
    from sirius_amd import _lib
    rows = 1 << k
    assert rows % ROWS == 0
    sels, fixed, W1, W2 = inputs(field, nsel, nfix, nadv, seed, rows)
    big = inputs(field, nsel, nfix, nadv, seed, rows * tile) if tile > 1 else (sels, fixed, W1, W2)
    kbig = k + (tile.bit_length() - 1)
    assert 1 << kbig == rows * tile
    got = []
    nch = None
    for no_jit, kind in ((0, kinds[0]), (1, kinds[1])):
        if kind is None:
            continue
        with S.tuning(no_jit=no_jit):
            St = S.PlonkStructure(field, kbig, big[0], big[1], nadv, gates)
        try:
            sid = C.c_int()
            _lib.lib().srs_structure_program_source(St._h, 0, None, 0, None, C.byref(sid))
            assert (sid.value >= 0) if kind == "aot" else (sid.value == kind), ("kernel kind", sid.value, kind)
            nch = St.num_challenges
            u1c, u1u, u2c = picks(field, nch, seed + 1), picks(field, 1, seed + 2)[0], picks(field, nch, seed + 3)
            terms, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, big[2], u2c, big[3])
            got.append((kind, [np.asarray(t) for t in terms]))
        finally:
            St.close()
    ch = S.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    _, exp = OE.cross_terms_oracle(O, field, [tuples(g) for g in gates], nsel, nfix, nadv, sels, fixed, W1, W2, ch)
    for kind, terms in got:
        assert len(terms) == len(exp), (kind, len(terms), len(exp))
        for i, (a, b) in enumerate(zip(terms, exp)):
            want = np.tile(b, (tile, 1)) if tile > 1 else b
            bad = np.flatnonzero(np.any(a != want, axis=1))
            assert bad.size == 0, (f"cross term {i + 1}, kernel kind {kind}: {bad.size} rows differ from the oracle, first rows", bad[:8].tolist())
    return len(exp)


def main_gate_oracle_gates(gate_T, nfix):
    from oracle import expr as OE
    og, fo, ao = [], 0, 0
    for T in gate_T:
        og.append(OE.main_gate_expression(T, 0, fo, ao, nfix)); fo += 2 * T + 5; ao += T + 2
    return og


def eval_gates_case(S, O, field, k, gate_T, seed):
    """srs_eval_gates of the MainGate list, homogeneous (the ahead-of-time kernel in sweep form with ONE point) and compressed, on
    word-set inputs against the oracle's GraphEvaluator program"""
    from oracle import expr as OE
    from workloads import gates_for
    gates, nfix, nadv = gates_for(gate_T)
    rows = 1 << k
    _, fixed, W1, _ = inputs(field, 0, nfix, nadv, seed, rows)
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    try:
        # (the homogeneous program is the cross-term program: the ahead-of-time kernel; the compressed one runs on the interpreter)
        assert program_source(St, 2)[1] >= 0, "expected the ahead-of-time kernel"
        cg = OE.CompressedGates.new(main_gate_oracle_gates(gate_T, nfix), OE.QueryIndexContext(0, nfix, nadv, 0, 0))
        p = P.MODULI[field]
        nch = St.num_challenges
        ch = picks(field, nch, seed + 4)
        chh = np.concatenate([ch, picks(field, 1, seed + 5)])
        for hom, expr, c in ((False, cg.compressed, ch), (True, cg.homogeneous, chh)):
            want = O.eval_program(field, OE.GraphEvaluator(expr, p).export(field, O), [], fixed, W1, None, c)
            assert np.array_equal(St.eval_gates(W1, c, homogeneous=hom), want), ("eval_gates", gate_T, "homogeneous" if hom else "compressed")
    finally:
        St.close()


def pg_case(S, O, k, gate_T, compat, seed=6):
    """ProtoGalaxy compute_F, compute_G, evaluate_e (and prove's K, whose G skips the points 0 and 1) of the MainGate list with one incoming
    trace: witnesses, fixed columns, betas and delta from the word set, against oracle.protogalaxy"""
    from oracle import protogalaxy as OPG
    from sirius_amd import protogalaxy as PG
    from workloads import gates_for
    gates, nfix, nadv = gates_for(gate_T)
    rows = 1 << k
    _, fixed, W0, W1 = inputs(0, 0, nfix, nadv, seed, rows)
    Ws = [W0, W1]
    St = S.PlonkStructure(0, k, [], fixed, nadv, gates)
    try:
        ctx = PG.PolyContext(St, 1)
        oS = OPG.Structure(O, main_gate_oracle_gates(gate_T, nfix), k, [], fixed, nadv, 0)
        octx = oS.context(1)
        ints = lambda a: O.mont_to_ints(O.FR, np.ascontiguousarray(a).reshape(-1, 4))
        betas, delta = picks(0, ctx.betas_count, seed + 1), picks(0, 1, seed + 2)[0]
        betas_i, delta_i = ints(betas), ints(delta)[0]
        alpha_i, gamma_i = word_ints(0)[3], word_ints(0)[7]
        m = lambda v: O.ints_to_mont(O.FR, list(v))
        eF = (OPG.compute_F if compat else OPG.compute_F_fast)(oS, octx, betas_i, delta_i, Ws[0], [], compat)
        bs = OPG.beta_stroke(betas_i, alpha_i, delta_i)
        eG = (OPG.compute_G if compat else OPG.compute_G_fast)(oS, octx, bs, Ws, [[], []], compat)
        ee = (OPG.evaluate_e_from_trace if compat else OPG.evaluate_e_fast)(oS, octx, betas_i, Ws[1], [], compat)
        eK = OPG.compute_K_from_G(octx, eG, OPG.poly_eval(eF, alpha_i))
        assert ints(PG.compute_F(ctx, betas, delta, Ws[0], reference_compat=compat)) == eF, "compute_F"
        assert ints(PG.compute_G(ctx, m(bs), Ws, reference_compat=compat)) == eG, "compute_G"
        assert ints(PG.evaluate_e_from_trace(ctx, betas, Ws[1], reference_compat=compat)) == [ee], "evaluate_e"
        import torch              # srs_pg_prove takes DEVICE pointers (there is no space argument): device-resident on a GPU, host on the emulator
        dWs = [torch.from_numpy(w.view(np.int64)).cuda() for w in Ws] if torch.cuda.is_available() else Ws
        pr = PG.prove(ctx, betas, delta, dWs, alpha=m([alpha_i])[0], gamma=m([gamma_i])[0], reference_compat=compat, fold=False)
        assert ints(pr["poly_F"]) == eF and ints(pr["poly_K"]) == eK, "prove: F, K"
    finally:
        St.close()


def fold_case(S, O, field, n=257, seed=8):
    """fold_witness, fold_error and fold_lincomb on n words of the set"""
    from oracle import protogalaxy as OPG
    from sirius_amd import protogalaxy as PG
    p = P.MODULI[field]
    W = words(field)
    rng = np.random.default_rng(seed)
    vec = lambda: np.ascontiguousarray(W[rng.integers(0, W.shape[0], size=n)])
    ints = lambda a: O.mont_to_ints(field, np.ascontiguousarray(a).reshape(-1, 4))
    W1, W2, E = vec(), vec(), vec()
    terms = [vec() for _ in range(3)]
    r = picks(field, 1, seed + 1)[0]
    ri = ints(r)[0]
    acc = S.RelaxedPlonkWitness(field, [W1.copy()], E.copy()).fold([W2], terms, r)
    assert ints(acc.W[0]) == [(a + ri * b) % p for a, b in zip(ints(W1), ints(W2))], "fold_witness"
    want = ints(E)
    for j, t in enumerate(terms):
        want = [(e + pow(ri, j + 1, p) * x) % p for e, x in zip(want, ints(t))]
    assert ints(acc.E) == want, "fold_error"
    coefs = picks(field, 3, seed + 2)
    ci = ints(coefs)
    Ws = [vec() for _ in range(3)]
    got = PG.fold_witness(field, Ws, coefs)
    wi = [ints(w) for w in Ws]
    assert ints(got) == [sum(c * w[i] for c, w in zip(ci, wi)) % p for i in range(n)], "fold_lincomb"
