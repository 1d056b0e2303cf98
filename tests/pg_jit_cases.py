"""Shared cases of the ProtoGalaxy leaf kernels compiled at run time, for the GPU (tests/test_pg_jit_gpu.py) and the logic
emulator (tests/test_pg_jit_emu.py).  Every case runs with the intended leaf rows (reference_compat=False) on a structure whose leaf kernels
were compiled with `prepare_pg_leaves()` and on a twin created under `tuning(no_jit=1)`: kernel_kind(2) is 2 on the first and 0 on the twin
(1 where the twin has ahead-of-time kernels: the `pg_jit_force` cases), and both equal the oracle, value for value -- hence each other, byte for byte: every output is a canonical
Montgomery element.  One structure is compiled per case where the shared case functions allow it (hiprtc takes seconds)."""
import contextlib
import random

import numpy as np


class Structures:
    """Stands in for the `sirius_amd` module in the shared case functions (pg_cases.run_pg_case, pg_route_cases): every PlonkStructure
    they create gets its leaf kernels compiled (`prepare`), and kernel_kind(2) is recorded after creation and again when it is closed."""

    def __init__(self, S, prepare):
        self._S, self.prepare, self.kinds, self.seconds = S, prepare, [], []

    def __getattr__(self, name):
        return getattr(self._S, name)

    def PlonkStructure(self, *a, **kw):
        St = self._S.PlonkStructure(*a, **kw)
        if self.prepare:
            self.seconds.append(St.prepare_pg_leaves())
        self.kinds.append(St.kernel_kind(2))
        close = St.close

        def recording_close():
            if getattr(St, "_h", None):
                self.kinds.append(St.kernel_kind(2))
            close()
        St.close = recording_close
        return St


@contextlib.contextmanager
def pair(S, force=False):
    """-> (run, kinds): run(fn) calls fn(module stand-in) once with compiled leaf kernels and once on the interpreter / ahead-of-time twin"""
    compiled, twin = Structures(S, True), Structures(S, False)

    def run(fn):
        with S.tuning(**({"pg_jit_force": 1} if force else {})):
            a = fn(compiled)
        with S.tuning(no_jit=1):
            b = fn(twin)
        return a, b
    yield run, (compiled, twin)
    assert compiled.kinds and set(compiled.kinds) == {2}, ("compiled leaf kernels expected", compiled.kinds)
    assert twin.kinds and set(twin.kinds) == {1 if force else 0}, ("the twin must not be compiled", twin.kinds)


def _products(S, O, k, gates, nfix, nadv, L, seed, nsel=0, nch=0):
    """F, G, e and prove (given alpha, gamma) of one structure on inputs that depend on the arguments alone"""
    from sirius_amd import protogalaxy as PG
    from oracle import pyref as P
    from workloads import rand_fe
    rows = 1 << k
    rng = np.random.default_rng(seed)
    rnd = random.Random(seed)
    fixed = [rand_fe(rng, rows, 0.3) for _ in range(nfix)]
    sels = [(rng.random(rows) < 0.7).astype(np.uint8) for _ in range(nsel)]
    Ws = [rand_fe(rng, nadv * rows) for _ in range(L + 1)]
    St = S.PlonkStructure(0, k, sels, fixed, nadv, gates)
    ctx = PG.PolyContext(St, L)
    m = lambda v: O.ints_to_mont(O.FR, list(v))
    betas_i = [rnd.randrange(P.FR) for _ in range(ctx.betas_count)]
    delta_i, alpha_i, gamma_i = (rnd.randrange(P.FR) for _ in range(3))
    chs_i = [[rnd.randrange(P.FR) for _ in range(nch)] for _ in Ws]
    chs = [m(c) if nch else np.zeros((0, 4), np.uint64) for c in chs_i]
    betas, delta = m(betas_i), m([delta_i])[0]
    chl = chs if nch else None
    out = dict(F=PG.compute_F(ctx, betas, delta, Ws[0], challenges=chs[0], reference_compat=False),
               G=PG.compute_G(ctx, betas, Ws, challenges_list=chl, reference_compat=False),
               e=PG.evaluate_e_from_trace(ctx, betas, Ws[-1], challenges=chs[-1], reference_compat=False))
    import torch
    dWs = [torch.from_numpy(w.view(np.int64)).cuda() for w in Ws] if torch.cuda.is_available() else Ws
    pr = PG.prove(ctx, betas, delta, dWs, alpha=m([alpha_i])[0], gamma=m([gamma_i])[0], challenges_list=chl, reference_compat=False)
    for name in ("poly_F", "poly_K", "betas_stroke", "e"):
        out["prove." + name] = np.ascontiguousarray(pr[name])
    St.close()
    out["inputs"] = dict(sels=sels, fixed=fixed, Ws=Ws, betas=betas_i, delta=delta_i, chs=chs_i)
    return out


def _equal(a, b):
    for name in a:
        if name != "inputs":
            assert np.array_equal(a[name], b[name]), f"{name}: compiled leaf kernels != twin"


def run_main_gate_case(S, O, k, gate_T, L, force=False):
    """MainGate lists through pg_cases.run_pg_case (every prover polynomial against the literal oracle, `prove` as one call included -- with
    one incoming trace that is integer-point G with F(alpha) at X = 1 inside `prove`) on both structures of the pair"""
    from pg_cases import run_pg_case
    with pair(S, force) as (run, _):
        run(lambda M: run_pg_case(M, O, k, gate_T, L, False))


def run_high_degree_case(S, O, k, d):
    """MainGate<2> plus a monomial of degree d > 8: more than DMAX + 1 integer points, the `run` form per point"""
    from pg_cases import high_degree_gates, run_pg_case
    with pair(S) as (run, _):
        run(lambda M: run_pg_case(M, O, k, None, 1, False, gates=high_degree_gates(d), ro_check=False))


def _has(e, kind, pred=lambda e: True):
    return (e[0] == kind and pred(e)) or any(isinstance(x, tuple) and _has(x, kind, pred) for x in e[1:])


def random_gate(nsel=1, nfix=2, nadv=2, seed=2031):
    """one gate from the generator of tests/test_emu_jit.py with a selector, a challenge and a rotated advice query, degree 2 .. 5: the first
    such expression of the seeded stream"""
    from oracle import expr as OE
    from test_emu_jit import _random_expr
    rnd = random.Random(seed)
    ctx = OE.QueryIndexContext(nsel, nfix, nadv, 0, 0)
    for _ in range(4000):
        g = _random_expr(rnd, nsel, nfix, nadv, 4)
        if not (_has(g, "chal") and _has(g, "poly", lambda e: e[1] < nsel) and _has(g, "poly", lambda e: e[1] >= nsel + nfix and e[2] != 0)):
            continue
        try:
            d = OE.homogeneous(g, ctx)[1]
        except Exception:
            continue
        if 2 <= d <= 5:
            return g
    raise AssertionError("no such gate in the stream")


def run_random_gate_case(S, O, k):
    """the random gate: F, G and e of the pair byte-equal, and equal to the oracle's literal restatement"""
    from oracle import protogalaxy as OPG
    nsel, nfix, nadv = 1, 2, 2
    gate = random_gate(nsel, nfix, nadv)
    with pair(S) as (run, _):
        a, b = run(lambda M: _products(M, O, k, [gate], nfix, nadv, 1, seed=5, nsel=nsel, nch=1))
        _equal(a, b)
    i = a["inputs"]
    oS = OPG.Structure(O, [gate], k, i["sels"], i["fixed"], nadv, 1)
    octx = oS.context(1)
    ints = lambda x: O.mont_to_ints(O.FR, np.ascontiguousarray(x).reshape(-1, 4))
    assert ints(a["F"]) == OPG.compute_F(oS, octx, i["betas"], i["delta"], i["Ws"][0], i["chs"][0], False), "compute_F"
    assert ints(a["G"]) == OPG.compute_G(oS, octx, i["betas"], i["Ws"], i["chs"], False), "compute_G"
    assert ints(a["e"]) == [OPG.evaluate_e_from_trace(oS, octx, i["betas"], i["Ws"][-1], i["chs"][-1], False)], "evaluate_e"


def run_sharded_case(S, O, k, gate_T, world, cache):
    """pg_route_cases.run_sharded_true_rows_case (the ranks' parts add up to the unsharded result, which equals the oracle) on both"""
    from pg_route_cases import run_sharded_true_rows_case
    with pair(S) as (run, _):
        run(lambda M: run_sharded_true_rows_case(M, O, k, world, gate_T, world, cache.setdefault(M.prepare, {})))
