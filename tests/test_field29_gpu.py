"""The DEVICE bodies of the field and curve arithmetic at their bounds: Fp29::mul / mul2 / sqr as generated into field29_chain.inc (chained
v_mad_u64_u32), Fp::mul as generated into field_fips.inc (96-bit columns with vcc carries), and everything of field29.cuh / curve29.cuh
built on them, madd_signed_fast and its sticky flag included -- run on the GPU by tests/devcalc (one thread per case, the product's
headers, the product's flags) on the vectors of tests/field29_cases.py, the very ones tests/test_field29_host.py runs through the plain
C++ twins.  Every result is judged twice: by Python integers (congruence, value bound, limb bounds), and word for word against the host
calculator on the same operands.  On top, what a line-by-line calculator cannot afford: BULK seeded cases per operation and field drawn
inside the stated bounds (Python integers only), and 4 096 random chains per curve whose exceptions fall at random positions.

What this does not prove.  The calculator inlines the generated bodies into kernels of its own; register allocation and scheduling around
the asm statements inside k_accum0s or k_ntt_pass_lazy are the compiler's and may differ there.  The asm constraints ("+&v", "s", the vcc
clobber) are what make that safe, and the pipeline tests on random inputs remain the check of those kernels as compiled.  This file adds
the arithmetic of the device bodies on the inputs random data never produces.  The run-time compiled row programs (csrc/jit.hip) compile
field.cuh / field29.cuh once more through hiprtc with flags of their own: not covered beyond tests/test_jit_gpu.py.

Cost (Python side; the launches themselves are milliseconds): see BULK below."""
import ctypes
import time

import numpy as np
import pytest

import field29_cases as FC
from field29_cases import CURVES, FIELDS

pytestmark = pytest.mark.gpu

# Cases per operation and field of the bulk layer.  The issue behind this file asks for 2^16 and lets the number shrink -- never the edge
# cases -- so that the GPU suite grows by no more than a tenth (about 36 s): generating and checking one case costs about 25 us of Python,
# 26 (operation, field) batches of 2^16 would cost some 45 s, 2^14 costs 11 s.
BULK = 1 << 14


class Device:
    def __init__(self):
        self.lib = ctypes.CDLL(FC.devcalc_build().build())
        self.lib.devcalc_run.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint, ctypes.c_uint, ctypes.c_uint, ctypes.c_void_p, ctypes.c_uint,
                                         ctypes.c_void_p, ctypes.c_uint]
        self.launches = 0

    def batch(self, op, which, cp, e, cases):
        """one launch: cases of ONE operation (and one (cp, e)) -> their results as lists of words"""
        wi = FC.chain_in_words(op, max(len(c.seq) for c in cases)) if op in FC.CHAIN_OPS else FC.IN_WORDS[op]
        wo = FC.OUT_WORDS[op]
        a = np.array([FC.dev_words(c, wi) for c in cases], dtype=np.uint32)
        assert a.shape == (len(cases), wi)
        out = np.full((len(cases), wo), 0xDEADBEEF, dtype=np.uint32)
        rc = self.lib.devcalc_run(op.encode(), which.encode(), cp, e, len(cases), a.ctypes.data, wi, out.ctypes.data, wo)
        assert rc == 0, f"devcalc_run({op}, {which}, {cp}, {e}) returned {rc}"
        self.launches += 1
        return out.tolist()

    def run(self, cases):
        """any mix of cases, one launch per (operation, field / curve, cp, e); results in the order of `cases`"""
        groups = {}
        for i, c in enumerate(cases):
            groups.setdefault((c.op, c.which, c.cp, c.e), []).append(i)
        res = [None] * len(cases)
        for (op, which, cp, e), idx in groups.items():
            for i, r in zip(idx, self.batch(op, which, cp, e, [cases[i] for i in idx])):
                res[i] = r
        return res


@pytest.fixture(scope="module")
def dev():
    d = Device()
    assert d.lib.devcalc_info() == 3
    return d


@pytest.fixture(scope="module")
def calc():
    ask, close = FC.host_calculator()
    yield ask
    close()


def first_wrong(c, got, ref):
    i = next(j for j in range(len(ref)) if got[j] != ref[j])
    return f"{c!r}: first wrong word {i}: device {got[i]:x}, host {ref[i]:x}"


def judge(dev, calc, cases):
    """device results of `cases`: each against Python integers, each word for word against the host calculator on the same operands"""
    got = dev.run(cases)
    for c, r in zip(cases, got):
        FC.check(c, r)
        ref = calc(FC.host_line(c))
        assert r == ref, first_wrong(c, r, ref)
    return got


def also_called(cases):
    """mul / sqr / mul8 also through the noinline wrappers: operands and result pass through the calling convention, as in the row programs"""
    return cases + [c.retarget(c.op + "_ni") for c in cases if c.op in ("mul", "sqr", "mul8")]


@pytest.mark.parametrize("name,p", FIELDS)
def test_products_at_the_bounds(dev, calc, name, p):
    cases = also_called(FC.product_cases(name, p))
    judge(dev, calc, cases)
    n = FC.counts(cases)
    assert n["mul_ni"] == n["mul"] >= 964 and n["sqr_ni"] == n["sqr"] >= 432 and n["mul2"] >= 1217
    print(f"\n{name}: {sorted(n.items())}")


@pytest.mark.parametrize("name,p", FIELDS)
def test_lazy_sums_differences_and_reductions(dev, calc, name, p):
    cases = FC.lazy_cases(name, p)
    judge(dev, calc, cases)
    assert set(FC.counts(cases)) == {"norm", "add", "sub", "neg", "canon", "redlazy", "unpack", "pack"}


@pytest.mark.parametrize("name,p", FIELDS)
def test_fp_mul_8x32(dev, calc, name, p):
    """the FIPS body on the operand domain stated above Fp::mul in field.cuh, inlined and called"""
    judge(dev, calc, also_called(FC.mul8_cases(name, p)))


@pytest.mark.parametrize("cname,cid", CURVES)
def test_group_law_on_the_lazy_form(dev, calc, cname, cid):
    G = FC.GroupCases(cname, cid)
    p = G.cv.p
    judge(dev, calc, G.tform_cases())
    a, b = judge(dev, calc, G.chain_cases("chain")), judge(dev, calc, G.chain_cases("chains"))
    for (label, _), ra, rb in zip(G.seqs, a, b):
        assert FC.same_record_or_point(ra, rb, p), label
    c = judge(dev, calc, G.stage2({label: r for (label, _), r in zip(G.seqs, b)}))       # operands: the records the DEVICE produced
    judge(dev, calc, [FC.xyzz_case(cname, p, r) for r in a + b + c])


@pytest.mark.parametrize("cname,cid", CURVES)
def test_chain_as_the_bucket_accumulation_runs_it(dev, calc, cname, cid):
    G = FC.GroupCases(cname, cid)
    p = G.cv.p
    fast = G.chainf_cases("chainf")
    got = judge(dev, calc, fast)
    plain = [c for c in fast if not c.want[1] and c.init is None]
    ref = dev.run([FC.Case("chains", cname, seq=c.seq) for c in plain])
    for c, r in zip(plain, ref):
        assert FC.same_record_or_point(got[fast.index(c)][:32], r, p), c
    raw = G.chainf_cases("chainf_raw")                      # the "garbage within the bounds" after an exception, and one and two additions later
    judge(dev, calc, raw)
    assert sum(1 for c in raw if c.want[1]) >= 30


BULK_OPS = ("mul", "sqr", "mul2", "norm", "add", "sub", "neg", "canon", "redlazy", "unpack", "pack", "mul8")


@pytest.mark.parametrize("name,p", FIELDS)
def test_bulk_inside_the_bounds(dev, name, p):
    """BULK seeded cases per operation, values hugging the bounds (k p + {0, 1, p - 1, p / 2, random}), limbs re-distributed at random:
    Python integers only.  mul / sqr / mul8 run inlined and called on the same operands."""
    t0 = time.time()
    for k, op in enumerate(BULK_OPS):
        cases = also_called(FC.bulk_cases(op, name, p, BULK, 1000 * k + len(name) + p % 97))
        for c, r in zip(cases, dev.run(cases)):
            FC.check(c, r)
    print(f"\n{name}: {len(BULK_OPS)} operations x {BULK} cases in {time.time() - t0:.1f} s, {dev.launches} launches so far")


@pytest.mark.parametrize("cname,cid", CURVES)
def test_random_chains(dev, cname, cid):
    """4 096 seeded chains of 1 .. 64 additions over 12 points, their negatives and the identity entry, half of them on top of a packed partial
    sum: through madd (chain), madd_signed (chains) -- both complete, from the identity -- and the accumulation's fast phase (chainf, with
    its `init`), whose flag must be the Python prediction for EVERY chain and whose point must be right wherever the flag is 0.  The
    generator asserts that 20 .. 80 % of the chains are exceptional, with every kind of exception present."""
    p = FC.P.CURVES[cid].p
    cases, kinds = FC.random_chain_cases(cname, cid)
    full, complete, fast = cases["chain"], cases["chains"], cases["chainf"]
    assert len(full) == len(complete) == len(fast) == 4096 and sum(1 for c in fast if c.init is not None) == 2048
    ra, rb, rf = dev.run(full), dev.run(complete), dev.run(fast)
    for i in range(len(fast)):
        FC.check(full[i], ra[i])
        assert rb[i] == ra[i] or FC.point_of(rb[i], p) == complete[i].want, complete[i]
        FC.check(fast[i], rf[i])
        if not fast[i].want[1] and fast[i].init is None:
            assert rf[i][:32] == rb[i], fast[i]             # no exception: the fast phase IS madd_signed, word for word
    print(f"\n{cname}: {kinds}")
