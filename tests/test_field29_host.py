"""The lazy 9 x 29-bit arithmetic of the hot kernels (csrc/field29.cuh, csrc/curve29.cuh) and Fp::mul (csrc/field.cuh) checked on the HOST
against Python integers, with operands sitting AT the bounds the headers state: limbs up to 2^31 - 1, values up to 12 p, differences
with the offsets the curve code uses, exceptional cases of the group law (identity operands, Q = +-acc), the chain as the bucket
accumulation runs it (madd_signed_fast and its sticky flag).  tests/emu/field29_check.cpp compiles the headers' plain C++ bodies with g++
through the emulator headers; the vectors and their expectations are tests/field29_cases.py, which tests/test_field29_gpu.py runs through
the generated device bodies as well.  Every test prints its per-operation case counts (pytest -s)."""
import pytest

import field29_cases as FC
from field29_cases import CURVES, FIELDS

# cases per operation and field / curve that this file ran before the vectors moved into field29_cases.py: the shared set must not go below
FLOOR = {"mul": 964, "mul2": 1217, "sqr": 432, "norm": 33, "add": 33, "sub": 446, "neg": 446, "canon": 109, "redlazy": 636, "unpack": 5, "pack": 5,
         "chain": 14, "chains": 14, "addp": 6, "dblp": 2, "tform": 72, "xyzz": 20}


@pytest.fixture(scope="module")
def calc():
    ask, close = FC.host_calculator()
    yield ask
    close()


def run(calc, cases, ran):
    out = []
    for c in cases:
        r = calc(FC.host_line(c))
        FC.check(c, r)
        ran[c.op] = ran.get(c.op, 0) + 1
        out.append(r)
    return out


def floor_ok(name, ran):
    print(f"\n{name}: cases per operation {sorted(ran.items())}")
    for op, n in ran.items():
        assert n >= FLOOR.get(op, 0), (op, n)


@pytest.mark.parametrize("name,p", FIELDS)
def test_products_at_the_bounds(calc, name, p):
    ran = {}
    run(calc, FC.product_cases(name, p), ran)
    assert set(ran) == {"mul", "mul2", "sqr"}
    floor_ok(name, ran)


@pytest.mark.parametrize("name,p", FIELDS)
def test_lazy_sums_differences_and_reductions(calc, name, p):
    ran = {}
    run(calc, FC.lazy_cases(name, p), ran)
    assert set(ran) == {"norm", "add", "sub", "neg", "canon", "redlazy", "unpack", "pack"}
    floor_ok(name, ran)


@pytest.mark.parametrize("name,p", FIELDS)
def test_fp_mul_8x32(calc, name, p):
    """Fp::mul on the operand domain stated above it in field.cuh -- here the host 4 x 64 CIOS."""
    ran = {}
    run(calc, FC.mul8_cases(name, p), ran)
    floor_ok(name, ran)


@pytest.mark.parametrize("cname,cid", CURVES)
def test_group_law_on_the_lazy_form(calc, cname, cid):
    G = FC.GroupCases(cname, cid)
    p = G.cv.p
    ran = {}
    run(calc, G.tform_cases(), ran)                         # ABI affine -> table form through the library
    # every sequence through Ec29::madd(load(..)) AND madd_signed(load_raw(..)): packed records are canonical except for the scale of
    # (zz, zzz) -- where they differ, the points are compared
    a, b = run(calc, G.chain_cases("chain"), ran), run(calc, G.chain_cases("chains"), ran)
    for (label, _), ra, rb in zip(G.seqs, a, b):
        assert FC.same_record_or_point(ra, rb, p), label
    records = {label: r for (label, _), r in zip(G.seqs, b)}
    # full additions / doublings of packed partial sums (what the accumulation levels and the bucket reduction run on)
    second = G.stage2(records)
    c = run(calc, second, ran)
    run(calc, [FC.xyzz_case(cname, p, r) for r in a + b + c], ran)       # packed R'-form -> ABI XYZZ (to_xyzz)
    floor_ok(cname, ran)


@pytest.mark.parametrize("cname,cid", CURVES)
def test_chain_as_the_bucket_accumulation_runs_it(calc, cname, cid):
    """madd_signed_fast behind the first phase of accumulate_part: without an exception exc == 0, the point is the Python sum and the record is
    the one `chains` gives; with Q = +-acc, an identity entry or an identity accumulator exc == 1, and what the chain returns then -- and
    after one and two further additions -- stays within the accumulator's limb and value bounds."""
    G = FC.GroupCases(cname, cid)
    p = G.cv.p
    ran = {}
    fast = G.chainf_cases("chainf")
    got = run(calc, fast, ran)
    assert any(c.want[1] for c in fast) and any(not c.want[1] for c in fast)
    for c, r in zip(fast, got):
        if not c.want[1] and c.init is None:                # the complete formulas on the same sequence
            ref = calc(FC.host_line(FC.Case("chains", cname, seq=c.seq)))
            assert FC.same_record_or_point(r[:32], ref, p), c
    raw = G.chainf_cases("chainf_raw")
    run(calc, raw, ran)
    assert sum(1 for c in raw if c.want[1]) >= 30
    floor_ok(cname, ran)


@pytest.mark.parametrize("cname,cid", CURVES)
def test_random_chains_are_not_vacuous(calc, cname, cid):
    """The 4 096 random chains the GPU test runs: the generator's own conditions (20 .. 80 % exceptional, every kind of exception present)
    hold for the Python side alone, and the first 128 chains pass through the host calculator."""
    cases, kinds = FC.random_chain_cases(cname, cid)
    assert len(cases["chainf"]) == 4096
    ran = {}
    for op in ("chain", "chains", "chainf"):
        run(calc, cases[op][:128], ran)
    print(f"\n{cname}: {kinds}")
