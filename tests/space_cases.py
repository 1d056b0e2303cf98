"""Both memory spaces of every C-ABI entry that stages host operands (csrc/capi.hip, Staging), shared by the GPU twin
(tests/test_spaces_gpu.py: torch CUDA tensors) and the emulator twin (tests/test_spaces_emu.py: NumPy memory handed over as
SRS_SPACE_DEVICE -- NumPy memory IS the emulator's device memory).

Every case runs an entry with host operands, checks the result against the oracle where the oracle has the function, runs it again
with device operands and asserts the two outputs byte-identical.  Sizes: the arena pads every operand to 256 bytes = 8 field
elements, so the vector entries run at n = 1, 7, 8, 9 and 257 (the NTT, whose length is a power of two, at the same spans through its
batched form: row length + gap), the structure entries at k = 4 and 5 on a gate set with two cross terms and on one with a lookup.
`*_regrow_case`: small, larger, small again on ONE handle / thread -- where a grow-only arena grows between calls.

A twin hands the cases a `Spaces`: dev(array) -> the operand in device space, host(operand) -> NumPy (n, 4) uint64."""
import numpy as np

from oracle import expr as OE
from oracle import lookup as OL
from oracle import protogalaxy as OPG
from oracle import pyref as P
from workloads import gates_for, rand_fe

VECTOR_SIZES = (1, 7, 8, 9, 257)
NTT_SHAPES = ((0, 0, 1), (0, 2, 3), (3, 0, 1), (0, 3, 3), (0, 127, 3), (8, 1, 2))     # (log n, gap, batch): spans of 1, 7, 8, 9, 257 and 513 elements
STRUCTURE_KS = (4, 5)
MAIN_GATES = [5, 3]          # MainGate<5> + MainGate<3>: homogeneous degree >= 2, so at least two cross terms


class EmuDevice(np.ndarray):
    """NumPy memory that the emulator twin passes as SRS_SPACE_DEVICE (Spaces.emulator patches the mirror's _buf for it)."""


class Spaces:
    def __init__(self, dev, host, addr):
        self.dev, self.host, self.addr = dev, host, addr

    @staticmethod
    def torch_cuda():
        import torch

        def dev(a):
            a = np.ascontiguousarray(a)
            return torch.from_numpy(a if a.dtype == np.uint8 else a.view(np.int64)).cuda()

        def host(x):
            if not type(x).__module__.startswith("torch"):
                return np.asarray(x)
            torch.cuda.synchronize()                       # stream-ordered entries: the result is ready in stream order
            return x.cpu().numpy().view(np.uint64)
        return Spaces(dev, host, lambda x: x.data_ptr())

    @staticmethod
    def emulator(monkeypatch):
        """the mirror decides the space in _buf: EmuDevice arrays become SRS_SPACE_DEVICE there, everything else is as it was"""
        import sirius_amd.commitment as cm
        import sirius_amd.plonk as pk
        import sirius_amd.protogalaxy as pg
        plain = cm._buf

        def _buf(x, last):
            addr, space, n, keep = plain(x, last)
            return addr, (cm.L.SPACE_DEVICE if isinstance(x, EmuDevice) else space), n, x if isinstance(x, EmuDevice) else keep
        for mod in (cm, pk, pg):
            monkeypatch.setattr(mod, "_buf", _buf)

        def dev(a):
            a = np.ascontiguousarray(a)
            return a.copy().view(EmuDevice) if a.dtype != np.uint8 else a.copy()
        return Spaces(dev, lambda x: np.asarray(x).view(np.ndarray), lambda x: x.ctypes.data)


def _same(sp, got_dev, got_host, what):
    a, b = sp.host(got_dev), np.asarray(got_host)
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def _ints(rng, n, p):
    return [int(rng.integers(1, 1 << 62)) * int(rng.integers(1, 1 << 62)) % p for _ in range(n)]


# ---------------------------------------------------------------- vector entries
def fold_case(S, O, sp, field, n, n_terms):
    """srs_fold_witness, srs_fold_error (in place in the staged copy of their first input on host operands)"""
    rng = np.random.default_rng(100 * n + n_terms + field)
    w1, w2, E, r = rand_fe(rng, n), rand_fe(rng, n), rand_fe(rng, n), rand_fe(rng, 1)[0]
    terms = [rand_fe(rng, n) for _ in range(n_terms)]
    keep = [x.copy() for x in (w1, w2, E, *terms)]
    acc = S.RelaxedPlonkWitness(field, [w1], E).fold([w2], terms, r)
    assert np.array_equal(acc.W[0], O.fold_w(field, w1, w2, r)), (n, "fold_w")
    assert np.array_equal(acc.E, O.fold_e(field, E, terms, r) if n_terms else E), (n, n_terms, "fold_e")
    assert all(np.array_equal(a, b) for a, b in zip(keep, (w1, w2, E, *terms))), "an input was written"
    dacc = S.RelaxedPlonkWitness(field, [sp.dev(w1)], sp.dev(E)).fold([sp.dev(w2)], [sp.dev(t) for t in terms], r)
    _same(sp, dacc.W[0], acc.W[0], (n, "fold_w"))
    _same(sp, dacc.E, acc.E, (n, n_terms, "fold_e"))
    return acc.W[0], acc.E


def lincomb_case(S, O, sp, n, J):
    """srs_fold_lincomb (transient staging; on host operands the sum lands in the staged copy of W[0])"""
    from sirius_amd import protogalaxy as PG
    rng = np.random.default_rng(10 * n + J)
    Ws = [rand_fe(rng, n) for _ in range(J)]
    coefs = _ints(rng, J, P.FR)
    m = O.ints_to_mont(O.FR, coefs)
    got = PG.fold_witness(0, Ws, m)
    assert np.array_equal(got, OPG.fold_witness(O, Ws, coefs)), (n, J)
    _same(sp, PG.fold_witness(0, [sp.dev(w) for w in Ws], m), got, (n, J))


def lookup_hg_case(S, O, sp, field, n):
    """srs_lookup_coeff_2 (transient staging; synchronises in both spaces)"""
    p = P.MODULI[field]
    rng = np.random.default_rng(20 * n + field)
    l, t, r = _ints(rng, n, p), _ints(rng, n, p), _ints(rng, 1, p)[0]
    mult = [int(v) for v in rng.integers(0, 5, size=n)]
    want_h, want_g = OL.evaluate_h_g(l, t, r, mult, p)
    St = type("LookupOnly", (), {"field": field, "lookup_coeff_2": S.PlonkStructure.lookup_coeff_2})()
    lw, tw, mw = (O.ints_to_mont(field, v) for v in (l, t, mult))
    rw = O.ints_to_mont(field, [r])[0]
    hs, gs = St.lookup_coeff_2([lw], [tw], [mw], rw)
    assert O.mont_to_ints(field, hs[0]) == want_h and O.mont_to_ints(field, gs[0]) == want_g, (field, n)
    dh, dg = St.lookup_coeff_2([sp.dev(lw)], [sp.dev(tw)], [sp.dev(mw)], rw)
    _same(sp, dh[0], hs[0], (n, "h"))
    _same(sp, dg[0], gs[0], (n, "g"))


def assigned_case(S, O, sp, field, n):
    """srs_batch_invert_assigned, has_denominator null and non-null (a one-byte-per-element operand)"""
    p = P.MODULI[field]
    rng = np.random.default_rng(30 * n + field)
    num, den = _ints(rng, n, p), _ints(rng, n, p)
    has = rng.integers(0, 2, size=n).astype(np.uint8)
    has[0] = 1
    den[n // 2] = 0                                     # 1/0 := 0
    inv = lambda x: pow(x, p - 2, p) if x else 0
    numw, denw = O.ints_to_mont(field, num), O.ints_to_mont(field, den)
    for flags in (None, has):
        got = S.batch_invert_assigned(field, numw, denw, flags)
        want = [a * inv(d) % p if (flags is None or flags[i]) else a for i, (a, d) in enumerate(zip(num, den))]
        assert O.mont_to_ints(field, got) == want, (field, n, flags is None)
        _same(sp, S.batch_invert_assigned(field, sp.dev(numw), sp.dev(denw), None if flags is None else sp.dev(flags)), got, (n, flags is None))


def _ntt_batch(S, sp, x, n, stride, batch, inverse, coset, device):
    from sirius_amd import _lib as L
    from sirius_amd.commitment import _stream
    L.check(L.lib().srs_ntt_batch(L.FIELD_FR, sp.addr(x) if device else x.ctypes.data, n, stride, batch, inverse, coset,
                                  L.SPACE_DEVICE if device else L.SPACE_HOST, _stream()))


def ntt_case(S, O, sp, log_n, gap, batch):
    """srs_ntt_batch, in place: the staged span is (batch - 1) * stride + n elements, gaps between the rows included"""
    n = 1 << log_n
    stride = n + gap
    total = (batch - 1) * stride + n
    rng = np.random.default_rng(40 * n + gap + batch)
    a = O.to_mont(O.FR, rand_fe(rng, total))
    for inverse, coset, ref in ((0, 0, O.fft), (1, 1, O.coset_ifft)):
        want = a.copy()
        for b in range(batch):
            want[b * stride:b * stride + n] = ref(np.ascontiguousarray(a[b * stride:b * stride + n]))
        h = a.copy()
        _ntt_batch(S, sp, h, n, stride, batch, inverse, coset, False)
        assert np.array_equal(h, want), (n, gap, batch, inverse)           # the gaps come back as they went up
        d = sp.dev(a)
        _ntt_batch(S, sp, d, n, stride, batch, inverse, coset, True)
        _same(sp, d, h, (n, gap, batch, inverse))


def make_key(S, O, cid=0):
    """-> (key, bases): long enough for every commit of this module; one per twin"""
    bases = O.make_bases(cid, 11, 2 * max(VECTOR_SIZES) + 1)
    return S.CommitmentKey(cid, bases), bases


def commit_batch_case(S, O, sp, key, n, cid=0):
    """srs_commit_batch: three vectors of unequal lengths, one of them empty"""
    ck, bases = key
    vs = [rand_fe(np.random.default_rng(50 * n + i), ln, 0.3) for i, ln in enumerate((n, 0, 2 * n + 1))]
    got = ck.commit_batch(vs)
    for v, c in zip(vs, got):
        assert np.array_equal(c, O.msm(cid, v, bases[:len(v)]) if len(v) else np.zeros(8, np.uint64)), (n, len(v))     # empty: the identity (0, 0)
    assert np.array_equal(ck.commit_batch([sp.dev(v) for v in vs]), got), n
    return got


# ---------------------------------------------------------------- structure entries
def main_gate_case(S, O, sp, k, key=None, commit_forms=(True, False)):
    """srs_cross_terms / srs_commit_cross_terms (with T_out, and commitments only: the T vectors are staging temporaries),
    srs_eval_gates, srs_is_sat_gates (E null and non-null), srs_pg_compute_F / _G / srs_pg_evaluate_e, and the structure's arena
    growing and shrinking between them"""
    from sirius_amd import protogalaxy as PG
    field, rows = 0, 1 << k
    gates, nfix, nadv = gates_for(MAIN_GATES)
    og, fo, ao = [], 0, 0
    for T in MAIN_GATES:
        og.append(OE.main_gate_expression(T, 0, fo, ao, nfix)); fo += 2 * T + 5; ao += T + 2
    rng = np.random.default_rng(60 + k)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    W1, W2 = rand_fe(rng, nadv * rows), rand_fe(rng, nadv * rows)
    St = S.PlonkStructure(field, k, [], fixed, nadv, gates)
    assert St.num_cross_terms >= 2
    nch = St.num_challenges
    u1c, u1u, u2c = rand_fe(rng, nch), rand_fe(rng, 1)[0], rand_fe(rng, nch)
    # eval_gates first: the smallest staging of this structure (W + one row vector); the calls after it need more
    chh = np.concatenate([u1c, u1u.reshape(1, 4)])
    vals = St.eval_gates(W1, chh, homogeneous=True)
    _same(sp, St.eval_gates(sp.dev(W1), chh, homogeneous=True), vals, (k, "eval_gates"))
    # cross terms
    terms, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, W1, u2c, W2)
    ch = S.VanillaFS.cross_term_challenges(u1c, u1u, u2c, field)
    cg, exp = OE.cross_terms_oracle(O, field, og, 0, nfix, nadv, [], fixed, W1, W2, ch)
    assert len(terms) == cg.degree == St.num_cross_terms
    assert all(np.array_equal(a, b) for a, b in zip(terms, exp)), (k, "cross terms")
    dterms, _ = S.VanillaFS.commit_cross_terms(None, St, u1c, u1u, sp.dev(W1), u2c, sp.dev(W2))
    for a, b in zip(dterms, terms):
        _same(sp, a, b, (k, "cross terms"))
    if key is not None:
        ck, bases = key
        want = np.stack([O.msm(0, t, bases[:rows]) for t in exp])
        for want_terms in commit_forms:
            t_h, c_h = S.VanillaFS.commit_cross_terms(ck, St, u1c, u1u, W1, u2c, W2, want_terms=want_terms)
            t_d, c_d = S.VanillaFS.commit_cross_terms(ck, St, u1c, u1u, sp.dev(W1), u2c, sp.dev(W2), want_terms=want_terms)
            assert np.array_equal(c_h, want) and np.array_equal(c_d, want), (k, want_terms, "cross-term commitments")
            if want_terms:
                assert all(np.array_equal(a, b) for a, b in zip(t_h, exp))
                for a, b in zip(t_d, exp):
                    _same(sp, a, b, (k, "cross terms beside their commitments"))
    # the smallest staging again, after the arena has grown: the same gate values; then the deciders on them
    assert np.array_equal(St.eval_gates(W1, chh, homogeneous=True), vals), (k, "eval_gates after a larger call")
    for Wx, E, chx in ((W1, vals, chh), (W1, None, u1c)):
        bad = St.is_sat_gates(Wx, chx, E)
        assert St.is_sat_gates(sp.dev(Wx), chx, None if E is None else sp.dev(E)) == bad, (k, E is None)
        if E is not None:
            assert bad == 0
            Eb = E.copy()
            Eb[rows - 1] = rand_fe(rng, 1)[0]
            assert St.is_sat_gates(Wx, chx, Eb) == St.is_sat_gates(sp.dev(Wx), chx, sp.dev(Eb)) == 1
        else:
            comp = St.eval_gates(Wx, chx)
            _same(sp, St.eval_gates(sp.dev(Wx), chx), comp, (k, "compressed gate"))
            assert bad == int(np.count_nonzero(np.any(comp != 0, axis=1)))
    # ProtoGalaxy sums (srs_pg_*: J staged witnesses, the polynomial comes back in host memory in either space)
    ctx = PG.PolyContext(St, 1)
    oS = OPG.Structure(O, og, k, [], fixed, nadv, 0)
    octx = oS.context(1)
    betas, delta = _ints(rng, ctx.betas_count, P.FR), _ints(rng, 1, P.FR)[0]
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    for compat in (True, False):
        pF = PG.compute_F(ctx, m(betas), m([delta])[0], W1, reference_compat=compat)
        assert O.mont_to_ints(O.FR, pF) == OPG.compute_F(oS, octx, betas, delta, W1, [], compat), (k, compat, "F")
        assert np.array_equal(PG.compute_F(ctx, m(betas), m([delta])[0], sp.dev(W1), reference_compat=compat), pF)
        pG = PG.compute_G(ctx, m(betas), [W1, W2], reference_compat=compat)
        assert O.mont_to_ints(O.FR, pG) == OPG.compute_G(oS, octx, betas, [W1, W2], [[], []], compat), (k, compat, "G")
        assert np.array_equal(PG.compute_G(ctx, m(betas), [sp.dev(W1), sp.dev(W2)], reference_compat=compat), pG)
        pe = PG.evaluate_e_from_trace(ctx, m(betas), W1, reference_compat=compat)
        assert O.mont_to_ints(O.FR, pe) == [OPG.evaluate_e_from_trace(oS, octx, betas, W1, [], compat)], (k, compat, "e")
        assert np.array_equal(PG.evaluate_e_from_trace(ctx, m(betas), sp.dev(W1), reference_compat=compat), pe)
    assert np.array_equal(St.eval_gates(W1, chh, homogeneous=True), vals), (k, "eval_gates after the ProtoGalaxy sums")
    St.close()


def lookup_structure_case(S, O, sp, k, variant="scalar"):
    """srs_lookup_coeff_1 (3 outputs per lookup), srs_is_sat_log_derivative (W staged because the structure has lookups),
    srs_eval_gates / srs_is_sat_gates on a structure with lookup columns"""
    from lookup_cases import _circuit, _rand_fe, _shape, _sps_product, _to_product_expr
    X = S.expression
    field = 0
    p = P.MODULI[field]
    rows = 1 << k
    rng = np.random.default_rng(70 + k)
    ns, nf, na, ogates, olookups = _shape(variant)
    selectors, fixed, advice = _circuit(O, field, variant, k, rng)
    meta = OL.build_metainfo(k, ns, nf, na, ogates, olookups)
    St = S.PlonkStructure(field, k, selectors, fixed, na, [_to_product_expr(X, g) for g in ogates],
                          lookups=[([_to_product_expr(X, e) for e in i], [_to_product_expr(X, e) for e in t]) for i, t in olookups])
    assert St.num_lookups >= 1
    cols = advice()
    ch = _rand_fe(O, field, rng, St.num_challenges)
    W = _sps_product(S, St, cols, ch)                   # lookup_coeff_1 + lookup_coeff_2 on host operands
    We = OL.run_sps_witness(O, field, meta, selectors, fixed, cols, O.mont_to_ints(field, ch), p)
    assert len(W) == len(We) and all(np.array_equal(a, b) for a, b in zip(W, We)), (k, "sps witness")
    adv = np.ascontiguousarray(np.concatenate(cols))
    r1 = ch[0] if St.has_vector_lookup else np.zeros(4, np.uint64)
    host3 = St.lookup_coeff_1(adv, r1)
    dev3 = St.lookup_coeff_1(sp.dev(adv), r1)
    for hv, dv in zip(host3, dev3):
        for a, b in zip(dv, hv):
            _same(sp, a, b, (k, "lookup_coeff_1"))
    Wcat = np.ascontiguousarray(np.concatenate([w.reshape(-1, 4) for w in W]))
    prog_c = OE.GraphEvaluator(meta.compressed.compressed, p).export(field, O)
    vals = O.eval_program(field, prog_c, selectors, fixed, W, None, ch, num_advice=na, num_lookup=meta.num_lookups)
    got = St.eval_gates(W, ch)
    assert np.array_equal(got, vals), (k, "eval_gates")
    _same(sp, St.eval_gates(sp.dev(Wcat), ch), got, (k, "eval_gates"))
    bad = int(np.count_nonzero(np.any(vals != 0, axis=1)))
    assert St.is_sat_gates(W, ch) == St.is_sat_gates(sp.dev(Wcat), ch) == bad
    sat = OL.is_sat_log_derivative(O, field, meta, W, rows, p)
    assert (St.is_sat_log_derivative(W) == 0) == sat and St.is_sat_log_derivative(sp.dev(Wcat)) == St.is_sat_log_derivative(W)
    Wb = Wcat.copy()
    Wb[-rows + 3] = O.ints_to_mont(field, [12345])[0]   # one g value: the log-derivative sum of that lookup breaks
    assert St.is_sat_log_derivative(Wb) == St.is_sat_log_derivative(sp.dev(Wb)) == 1
    St.close()


def sparse_case(S, O, sp, n):
    """srs_sparse_matvec / srs_is_sat_permutation; permutation, matvec, permutation on one matrix: its arena grows for y"""
    field = 0
    p = P.MODULI[field]
    rng = np.random.default_rng(80 + n)
    nnz = 3 * n
    rows, cols = rng.integers(0, n, size=nnz).astype(np.uint64), rng.integers(0, n, size=nnz).astype(np.uint64)
    vals, Z = rand_fe(rng, nnz), rand_fe(rng, n)
    zi, vi = O.mont_to_ints(field, Z), O.mont_to_ints(field, vals)
    want = [0] * n
    for r, c, v in zip(rows, cols, vi):
        want[int(r)] = (want[int(r)] + v * zi[int(c)]) % p
    want = O.ints_to_mont(field, want)
    mism = int(np.count_nonzero(np.any(want != Z, axis=1)))
    M = S.SparseMatrix(field, n, rows, cols, vals)
    for device in (False, True):
        z = sp.dev(Z) if device else Z
        assert S.VanillaFS.is_sat_permutation(M, z) == mism, (n, device)
        _same(sp, M.matrix_multiply(z), want, (n, device, "matvec"))
        assert S.VanillaFS.is_sat_permutation(M, z) == mism, (n, device, "after the arena grew")
    M.close()


# ---------------------------------------------------------------- a grow-only arena across calls
def regrow_case(S, O, sp, key=None):
    """small, larger, small again: the thread's arena (folds, batch inversion) and, given a key, its staging arena"""
    small, large = 7, 257
    first = fold_case(S, O, sp, 0, small, 3)
    fold_case(S, O, sp, 0, large, 3)
    again = fold_case(S, O, sp, 0, small, 3)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    for n in (small, large, small):
        assigned_case(S, O, sp, 0, n)
    if key is None:
        return
    c0 = commit_batch_case(S, O, sp, key, small)
    commit_batch_case(S, O, sp, key, large)
    assert np.array_equal(commit_batch_case(S, O, sp, key, small), c0)
