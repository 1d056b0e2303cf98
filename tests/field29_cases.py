"""The vectors of the lazy 9 x 29-bit arithmetic (csrc/field29.cuh, csrc/curve29.cuh) and of Fp::mul (csrc/field.cuh), with their
Python-integer expectations -- ONE set for TWO executors: tests/test_field29_host.py runs them through the host build of the headers
(tests/emu/field29_check.cpp: the plain C++ bodies), tests/test_field29_gpu.py through tests/devcalc (the generated device bodies).

For every operation: a function that returns the cases (operands as limb lists, `bound` naming the bound a case sits at) and `check`,
which judges one result with Python integers alone.  The generators assert what makes the vectors worth running: the product cases reach
within 2 bits of the largest column sum the admissible operands allow, between 20 % and 80 % of the random chains are exceptional.

A case's operands are flat 32-bit words in the order the host calculator reads them (`host_line`); the device calculator takes the same
words (`dev_words`: chains are padded to a common length and always carry the 32 words of `init`)."""
import math
import os
import random
import subprocess

from oracle import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "tests", "emu")
R261 = 1 << 261
R256 = 1 << 256
M29 = (1 << 29) - 1
FIELDS = [("Fr", P.FR), ("Fq", P.FQ)]
CURVES = [("Bn256", 0), ("Grumpkin", 1)]
# the (CP, E) pairs of curve29.cuh, the sweep emitter and the NTT tile: the list of tests/emu/field29_calc.h (SRS_CALC_SUB_PAIRS)
SUB_PAIRS = ((1, 0), (2, 0), (3, 0), (5, 1), (6, 2), (7, 2), (8, 0), (10, 0), (13, 0), (31, 0), (3, 2), (12, 2), (6, 0), (8, 1))
ENTRY_WORDS = 17                 # a chain entry: 16 words of a table-form point and its sign
CHAIN_OPS = ("chain", "chains", "chainf", "chainf_raw")
IN_WORDS = {"mul": 18, "mul_ni": 18, "sqr": 9, "sqr_ni": 9, "mul2": 36, "norm": 9, "add": 18, "sub": 18, "neg": 9, "canon": 9, "redlazy": 9,
            "unpack": 8, "pack": 9, "mul8": 16, "mul8_ni": 16, "addp": 64, "dblp": 32, "tform": 16, "xyzz": 32}
OUT_WORDS = {"mul": 9, "mul_ni": 9, "sqr": 9, "sqr_ni": 9, "mul2": 9, "norm": 9, "add": 9, "sub": 9, "neg": 9, "canon": 8, "redlazy": 9,
             "unpack": 9, "pack": 8, "mul8": 8, "mul8_ni": 8, "chain": 32, "chains": 32, "chainf": 33, "chainf_raw": 37, "addp": 32, "dblp": 32,
             "tform": 16, "xyzz": 32}


def devcalc_build():
    """tests/devcalc/build.py as a module (build() -> the path of libdevcalc.so)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("devcalc_build", os.path.join(ROOT, "tests", "devcalc", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def host_calculator():
    """(ask, close) of the line-oriented host calculator, built when its sources changed.  ask(line) -> list of the result's words."""
    exe = devcalc_build().build_host()
    proc = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, bufsize=1)

    def ask(line):
        proc.stdin.write(line + "\n")
        proc.stdin.flush()
        out = proc.stdout.readline().strip()
        assert out and out != "unsupported", line[:80]
        return [int(x, 16) for x in out.split()]

    def close():
        proc.stdin.close()
        proc.wait(timeout=10)
    return ask, close


def limbs29(x, wide=0, rnd=None):
    """x -> 9 limbs of 29 bits (limb 8 takes the rest); wide: re-distribute so that limbs reach up to 2^(29+wide) - 1"""
    l = [(x >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [x >> 232]
    if wide:
        for i in range(8):
            room = ((1 << (29 + wide)) - 1 - l[i]) >> 29
            t = min(room, l[i + 1])
            if rnd is not None and t:
                t = rnd.randrange(t + 1)
            l[i] += t << 29
            l[i + 1] -= t
    assert all(0 <= v < (1 << 32) for v in l) and sum(v << (29 * i) for i, v in enumerate(l)) == x
    return l


val = lambda l: sum(v << (29 * i) for i, v in enumerate(l))
val32 = lambda l: sum(v << (32 * i) for i, v in enumerate(l))
hx = lambda l: " ".join(f"{v:x}" for v in l)
words = lambda x, n: [(x >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def edge_values(p, rnd, kmax):
    out = []
    for k in range(kmax + 1):
        for r in (0, 1, p - 1, p // 2, rnd.randrange(p)):
            v = k * p + r
            if v < (kmax + 1) * p and v < (1 << 260):
                out.append(v)
    return out


class Case:
    """One vector.  ins: the operand words (fixed-size operations); seq / init: a chain's entries [(16 words, neg)] and its packed partial sum
    (32 words or None); want: what `check` needs (integers, points); bound: the bound or the edge the case sits at."""
    __slots__ = ("op", "which", "cp", "e", "ins", "seq", "init", "want", "bound")

    def __init__(self, op, which, ins=None, want=None, bound="", cp=0, e=0, seq=None, init=None):
        self.op, self.which, self.ins, self.want, self.bound, self.cp, self.e, self.seq, self.init = op, which, ins, want, bound, cp, e, seq, init

    def retarget(self, op):
        """The same operands for another executor entry of the same operation (mul -> mul_ni ...)."""
        return Case(op, self.which, self.ins, self.want, self.bound, self.cp, self.e, self.seq, self.init)

    def __repr__(self):
        return f"<{self.op} {self.which} {self.bound} {host_line(self)[:400]}>"


def host_line(c):
    op = {"mul_ni": "mul", "sqr_ni": "sqr", "mul8_ni": "mul8"}.get(c.op, c.op)       # the called forms exist on the device only
    if op in CHAIN_OPS:
        body = f"{len(c.seq)} " + " ".join(hx(w) + f" {int(n)}" for w, n in c.seq)
        if op in ("chainf", "chainf_raw"):
            body = (f"1 {hx(c.init)} " if c.init is not None else "0 ") + body
        return f"{op} {c.which} {body}"
    if op in ("sub", "neg"):
        return f"{op} {c.which} {c.cp} {c.e} {hx(c.ins)}"
    return f"{op} {c.which} {hx(c.ins)}"


def chain_in_words(op, maxlen):
    return (1 if op in ("chain", "chains") else 34) + ENTRY_WORDS * max(1, maxlen)


def dev_words(c, in_words=None):
    """The case as the device calculator takes it: `in_words` words (chains: zero padded)."""
    if c.op not in CHAIN_OPS:
        assert len(c.ins) == IN_WORDS[c.op]
        return c.ins
    w = []
    if c.op in ("chainf", "chainf_raw"):
        w = [int(c.init is not None)] + (list(c.init) if c.init is not None else [0] * 32)
    w.append(len(c.seq))
    for ent, n in c.seq:
        w += list(ent) + [int(n)]
    assert len(w) <= in_words
    return w + [0] * (in_words - len(w))


# ---------------------------------------------------------------------------------------------------------------- products
def column_sums(pairs, p):
    """The column recurrence of the Montgomery product sum(a b) / 2^261 in radix 2^29, quotients included, exactly as field29.cuh states it
    -> (largest value the 64-bit column accumulator holds, the 9 result limbs)."""
    pl = limbs29(p)
    inv = (-pow(p, -1, 1 << 29)) % (1 << 29)
    acc, m, top, out = 0, [0] * 9, 0, []
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        acc += sum(a[i] * b[k - i] for a, b in pairs for i in range(lo, hi + 1))
        if k < 9:
            acc += sum(m[i] * pl[k - i] for i in range(k))
            m[k] = (acc * inv) & M29
            acc += m[k] * pl[0]
            top = max(top, acc)
            assert acc & M29 == 0
        else:
            acc += sum(m[i] * pl[k - i] for i in range(lo, 9))
            top = max(top, acc)
            out.append(acc & M29)
        acc >>= 29
    out.append(acc)
    return top, out


def column_upper_bound(p, widths, square=False):
    """An upper bound of the column accumulator over ALL admissible operands of a product: limbs a_i < 2^wa, b_j < 2^wb for each (wa, wb)
    of `widths` below the top limb, quotients m_i < 2^29, and the top limbs tied by the value bound sum(A B) < 2^261 p, which gives
    a_8 b_8 2^464 < 2^261 p.  A column is linear in a_8 and in b_8 and the admissible (a_8, b_8) lie under a hyperbola, so its maximum is at
    one of the two ends (a_8 at its limb bound, or b_8); for a square a_8 = b_8 <= sqrt.  Derived from the stated bounds only."""
    pl = limbs29(p)
    K = (R261 * p) >> 464
    ends = []
    for end in (0, 1):
        pairs = []
        for wa, wb in widths:
            amax, bmax = (1 << wa) - 1, (1 << wb) - 1
            if square:
                a8 = b8 = min(amax, math.isqrt(K) + 1)
            elif end == 0:
                a8, b8 = amax, min(bmax, K // amax + 1)
            else:
                b8, a8 = bmax, min(amax, K // bmax + 1)
            pairs.append(([amax] * 8 + [a8], [bmax] * 8 + [b8]))
        ends.append(pairs)
    bound, carry = 0, 0
    for k in range(17):
        lo, hi = max(0, k - 8), min(k, 8)
        terms = max(sum(a[i] * b[k - i] for a, b in pairs for i in range(lo, hi + 1)) for pairs in ends)
        s = carry + terms + sum(M29 * pl[k - i] for i in range(lo, hi + 1))
        bound = max(bound, s)
        carry = s >> 29
    return bound


def _fit_top(a, b_low, b8max, budget):
    """largest b_8 <= b8max with a * (b_low + b_8 2^232) < budget"""
    t = (budget - 1) // a - b_low
    assert t >= 0
    return min(b8max, t >> 232)


def _product_want(p, pairs):
    n = sum(val(a) * val(b) for a, b in pairs)
    assert n < R261 * p
    return n


_INV = {}


def _inv(radix, p):
    if (radix, p) not in _INV:
        _INV[radix, p] = pow(radix, -1, p)
    return _INV[radix, p]


def check_product(c, r, p):
    assert len(r) == 9 and all(v < (1 << 29) for v in r[:8]) and val(r) < 2 * p and val(r) % p == c.want * _inv(R261, p) % p, c


def product_cases(name, p):
    """mul / sqr / mul2.  First the cases this suite always had (seed 29: values k p + {0, 1, p - 1, p / 2, random} up to 12 p against the
    edge multipliers, limbs re-distributed up to 2^31 - 1 / 2^30 - 1; the bounds madd_signed feeds mul2), then the edges of the column
    sums: all-ones limbs at every admissible width combination with the top limbs taken from the value bound, zero limbs, equal operands."""
    rnd = random.Random(29)
    out = []

    def mul(la, lb, bound):
        out.append(Case("mul", name, la + lb, _product_want(p, [(la, lb)]), bound))

    def sqr(la, bound):
        out.append(Case("sqr", name, la, _product_want(p, [(la, la)]), bound))

    def mul2(la, lb, lc, ld, bound):
        out.append(Case("mul2", name, la + lb + lc + ld, _product_want(p, [(la, lb), (lc, ld)]), bound))

    cases = []
    big = edge_values(p, rnd, 12)
    for a in big[::3]:
        for b in (0, 1, p - 1, 2 * p - 1, 12 * p - 1, rnd.randrange(12 * p)):
            cases.append((a, b))
    cases += [(rnd.randrange(12 * p), rnd.randrange(12 * p)) for _ in range(300)]
    for a, b in cases:
        for wa in (0, 2):                                   # the wide operand: limbs < 2^31, the other normalised
            mul(limbs29(a, wa, rnd), limbs29(b), f"a<13p limbs<2^{29 + wa}, b<12p norm")
        sqr(limbs29(a, 1, rnd), "a<13p limbs<2^30")         # squares: limbs < 2^30
    for _ in range(100):                                    # both operands with limbs < 2^30
        a, b = rnd.randrange(12 * p), rnd.randrange(12 * p)
        mul(limbs29(a, 1, rnd), limbs29(b, 1, rnd), "both limbs<2^30")
    # mul2: (a b + c d) / 2^261 with ONE reduction -- a, c with limbs < 2^30, b, d normalised, at the bounds madd_signed uses
    # (t < 12P, r < 8P; 6P - y <= 6P, ppp < 2P) and at the extreme all-ones limb patterns
    quads = [(12 * p - 1, 8 * p - 1, 6 * p, 2 * p - 1), (0, 0, 0, 0), (p - 1, p - 1, p - 1, p - 1), (12 * p - 1, 8 * p - 1, 0, 0)]
    quads += [(rnd.randrange(12 * p), rnd.randrange(8 * p), rnd.randrange(6 * p + 1), rnd.randrange(2 * p)) for _ in range(300)]
    for a, b, c, d in quads:
        for wa, wc in ((0, 0), (1, 1), (0, 1), (1, 0)):
            la = limbs29(a, wa, rnd)
            mul2(la, limbs29(b), limbs29(c, wc, rnd), limbs29(d), f"madd_signed bounds, a limbs<2^{29 + wa}, c limbs<2^{29 + wc}")
    ones30, ones29 = [(1 << 30) - 1] * 8 + [(1 << 22) - 1], [(1 << 29) - 1] * 8 + [(1 << 21) - 1]      # every limb at its bound
    mul2(ones30, ones29, ones30, ones29, "all-ones 30/29, tops 2^22 / 2^21")

    # ---- the edges of the column sums.  All-ones below the top limb at each admissible width combination; the top limbs at both ends of
    # what the value bound A B (+ C D) < 2^261 p leaves (one at its limb bound, the other fitted), and with zero tops
    budget = R261 * p
    ones = lambda w, top: [(1 << w) - 1] * 8 + [top]
    for wa, wb in ((31, 29), (30, 30), (29, 29)):
        for end in (0, 1):
            if end == 0:
                la = ones(wa, (1 << wa) - 1)
                lb = ones(wb, _fit_top(val(la), val(ones(wb, 0)), (1 << wb) - 1, budget))
            else:
                lb = ones(wb, (1 << wb) - 1)
                la = ones(wa, _fit_top(val(lb), val(ones(wa, 0)), (1 << wa) - 1, budget))
            mul(la, lb, f"all-ones limbs<2^{wa} x limbs<2^{wb}, top limbs from the value bound (end {end})")
        mul(ones(wa, 0), ones(wb, 0), f"all-ones limbs<2^{wa} x limbs<2^{wb}, zero tops")
    root = math.isqrt(budget - 1)
    la = ones(30, min((1 << 30) - 1, (root - val(ones(30, 0))) >> 232))
    sqr(la, "all-ones limbs<2^30, top limb from the value bound")
    mul(la, la, "all-ones limbs<2^30, a = b, top limb from the value bound")
    sqr(ones(30, 0), "all-ones limbs<2^30, zero top")
    sqr(ones(29, (root - val(ones(29, 0))) >> 232), "all-ones norm, top limb from the value bound")
    for end in (0, 1):                                      # mul2: a, c < 2^30, b, d < 2^29, each product with half the budget
        if end == 0:
            la = ones(30, (1 << 30) - 1)
            lb = ones(29, _fit_top(val(la), val(ones(29, 0)), (1 << 29) - 1, budget // 2))
        else:
            lb = ones(29, (1 << 29) - 1)
            la = ones(30, _fit_top(val(lb), val(ones(30, 0)), (1 << 30) - 1, budget // 2))
        mul2(la, lb, la, lb, f"all-ones 30/29 twice (a = c, b = d), top limbs from the value bound (end {end})")
        mul2(la, lb, ones(30, 0), ones(29, 0), f"all-ones 30/29, second product with zero tops (end {end})")
    mul2(ones(30, 0), ones(29, 0), ones(30, 0), ones(29, 0), "all-ones 30/29 twice, zero tops")
    # zero limbs (constant-zero registers), equal operands (the pattern of the register-allocation accident recorded in tools/gen_field_fips.py)
    rz = random.Random(2929)
    zero_some = lambda l, keep: [v if (i in keep) else 0 for i, v in enumerate(l)]
    for a in edge_values(p, rz, 12)[1::4]:
        b = rz.choice([p - 1, 2 * p - 1, 12 * p - 1, rz.randrange(12 * p)])
        n, n2 = limbs29(a), limbs29(b)
        for keep in ((0,), (8,), (0, 8), (1, 3, 5, 7), (0, 2, 4, 6, 8), ()):
            mul(zero_some(limbs29(a, 2, rz), keep), n2, f"a with limbs {keep} only")
            mul(limbs29(b, 2, rz), zero_some(n, keep), f"b with limbs {keep} only")
            sqr(zero_some(limbs29(a, 1, rz), keep), f"a with limbs {keep} only")
            mul2(zero_some(limbs29(a, 1, rz), keep), limbs29(b % (8 * p)), limbs29(b % (6 * p), 1, rz), zero_some(limbs29(a % (2 * p)), keep),
                 f"a, d with limbs {keep} only")
        w1 = limbs29(a, 1, rz)
        mul(w1, w1, "a = b, limbs<2^30")
        mul(n, n, "a = b norm")
        a8, a2 = limbs29(a % (8 * p)), limbs29(a % (2 * p))
        mul2(a8, a8, a2, a2, "a = b, c = d norm")
        mul2(a8, a2, a8, a2, "a = c, b = d norm")
        mul2(a2, a2, a2, a2, "a = b = c = d norm")
        mul2(limbs29(a, 1, rz), a8, limbs29(a % (6 * p), 1, rz), a2, "a, b, c, d from one value")

    # the vectors sit AT the edge: per operation, some case comes within 2 bits of the largest column sum any admissible operand gives
    limits = {"mul": max(column_upper_bound(p, [w]) for w in ((31, 29), (30, 30))), "mul2": column_upper_bound(p, [(30, 29), (30, 29)]),
              "sqr": column_upper_bound(p, [(30, 30)], square=True)}
    reached = {"mul": 0, "mul2": 0, "sqr": 0}
    for c in out:
        l = [c.ins[9 * i: 9 * i + 9] for i in range(len(c.ins) // 9)]
        pairs = {"mul": lambda: [(l[0], l[1])], "sqr": lambda: [(l[0], l[0])], "mul2": lambda: [(l[0], l[1]), (l[2], l[3])]}[c.op]()
        top, res = column_sums(pairs, p)
        assert top < (1 << 64), c                                           # the header's "never leaves 64 bits", at these operands
        assert (val(res) * R261 - c.want) % p == 0 and val(res) < 2 * p, c      # the recurrence above is the product the header states
        reached[c.op] = max(reached[c.op], top)
    for op, lim in limits.items():
        assert lim < (1 << 64) and reached[op] * 4 >= lim, (op, reached[op].bit_length(), lim.bit_length())
    return out


# --------------------------------------------------------------------------------------------------- sums, differences, reductions
def check_lazy(c, r, p):
    op, w = c.op, c.want
    if op == "norm":
        assert val(r) == w and all(v < (1 << 29) for v in r[:8]), c
    elif op in ("add", "sub", "neg"):
        assert len(r) == 9 and all(v < (1 << 32) for v in r) and val(r) == w, c
    elif op == "canon":
        assert len(r) == 8 and val32(r) == w, c
    elif op == "redlazy":
        assert val(r) % p == w % p and val(r) < 2 * p and all(x < (1 << 29) for x in r[:8]), c
    elif op == "unpack":
        assert val(r) == w and all(x < (1 << 29) for x in r[:8]), c
    elif op == "pack":
        assert r == words(w, 8), c
    else:
        raise AssertionError(op)


def lazy_cases(name, p):
    rnd = random.Random(31)
    out = []
    vals = edge_values(p, rnd, 12)
    for a in vals[::2]:
        out.append(Case("norm", name, limbs29(a, 2, rnd), a, "a<13p limbs<2^31"))
        b = rnd.choice(vals)
        out.append(Case("add", name, limbs29(a, 1, rnd) + limbs29(b, 1, rnd), a + b, "limbs<2^30"))
    # a - b + CP p with the (CP, E) pairs of curve29.cuh and the sweep emitter; b below CP p with limbs < 2^(29 + E)
    for cp, e in SUB_PAIRS:
        for _ in range(40):
            b = rnd.choice([0, 1, p - 1, cp * p - 1, rnd.randrange(cp * p), max(0, cp * p - (1 << e) * (1 << 232))])
            lb = limbs29(b, e, rnd)
            top_ok = lb[8] <= ((cp * p) >> 232) - (1 << e)
            if not top_ok:
                continue
            a = rnd.randrange(12 * p)
            la = limbs29(a, 1, rnd)
            out.append(Case("sub", name, la + lb, a - b + cp * p, f"b<{cp}p limbs<2^{29 + e}", cp, e))
            out.append(Case("neg", name, lb, cp * p - b, f"b<{cp}p limbs<2^{29 + e}", cp, e))
    for v in [0, 1, p - 1, p, p + 1, 2 * p - 1, 2 * p, 3 * p, 4 * p - 1] + [rnd.randrange(4 * p) for _ in range(100)]:
        out.append(Case("canon", name, limbs29(v), v % p, "v<4p norm"))
    # r05 reduce_lazy (the NTT's closing reduction): any normalised value below 2^263 -> the same residue below 2P, normalised
    top = (1 << 263) - 1
    for v in ([0, 1, p - 1, p, p + 1, 2 * p, 469 * p, 469 * p - 1, 470 * p + 5, 700 * p, top, top - p, (1 << 232) - 1, 1 << 232, (1 << 262) + 12345]
              + [k * p + d for k in (1, 7, 29, 117, 235, 468, 600) for d in (-1, 0, 1)] + [rnd.randrange(top) for _ in range(300)]
              + [rnd.randrange(1, 720) * p + rnd.choice([0, 1, p - 1, rnd.randrange(p)]) for _ in range(300)]):
        v = min(v, top)
        out.append(Case("redlazy", name, limbs29(v), v, "v<2^263 norm"))
    for v in [0, 1, (1 << 256) - 1, p, rnd.randrange(1 << 256)]:
        out.append(Case("unpack", name, words(v, 8), v, "v<2^256"))
        out.append(Case("pack", name, limbs29(v), v, "v<2^256 norm"))
    return out


# ------------------------------------------------------------------------------------------------------------- Fp::mul, 8 x 32
def check_mul8(c, r, p):
    assert len(r) == 8 and val32(r) == c.want * _inv(R256, p) % p, c


def mul8_domain(a, b, p):
    """The operand domain stated above Fp::mul (csrc/field.cuh): a b < 2^256 p, a < 2^255, b < 2^256."""
    return a * b < R256 * p and a < (1 << 255) and b < R256


def mul8_cases(name, p, randoms=3000):
    rnd = random.Random(832)
    r2 = R256 * R256 % p
    ff = lambda n: (1 << (32 * n)) - 1                     # the n lowest 32-bit limbs all 0xFFFFFFFF
    # canonical values
    vs = [0, 1, R256 % p, p - 1, p - 2, r2, p // 2, ff(7) | (p >> 224 << 224), ff(7), ff(6), ff(4), ff(7) - ff(3), (p >> 224 << 224)]
    vs += [1 << (32 * i) for i in range(8) if (1 << (32 * i)) < p] + [(1 << (32 * i)) - 1 for i in range(1, 8)]
    vs += [(p - 1) & ~(0xFFFFFFFF << (32 * i)) for i in range(8)]                      # p - 1 with limb i zero
    vs += [v & 0xFFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000 for v in (p - 1, ff(7))]
    vs += [v & 0x00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF00000000FFFFFFFF for v in (p - 1, ff(8))]
    vs = [v for v in dict.fromkeys(vs) if v < p]
    out = []
    for a in vs:
        for b in vs:
            out.append(Case("mul8", name, words(a, 8) + words(b, 8), a * b, "canonical edge values" + (", a = b" if a == b else "")))
    for _ in range(randoms):
        a, b = rnd.randrange(p), rnd.randrange(p)
        out.append(Case("mul8", name, words(a, 8) + words(b, 8), a * b, "random canonical"))
    for _ in range(200):
        a = rnd.randrange(p)
        out.append(Case("mul8", name, words(a, 8) + words(a, 8), a * a, "random canonical, a = b"))
    # non-canonical operands inside the domain: p <= v < 2p on both sides; any 256-bit b against an a that keeps a b < 2^256 p
    nc = [p, p + 1, 2 * p - 1, 2 * p - 2, p + (p >> 1)] + [p + rnd.randrange(p) for _ in range(20)]
    for a in nc:
        for b in nc + [0, 1, p - 1]:
            out.append(Case("mul8", name, words(a, 8) + words(b, 8), a * b, "p <= operands < 2p"))
            out.append(Case("mul8", name, words(b, 8) + words(a, 8), a * b, "p <= operands < 2p"))
    for b in [R256 - 1, R256 - 2, ff(8) - ff(4), 1 << 255, (1 << 255) - 1] + [rnd.randrange(2 * p, R256) for _ in range(50)]:
        for a in [0, 1, 2, p - 1, p - 2, (R256 * p - 1) // b, rnd.randrange(p), 1 << 32, 1 << 224]:
            if mul8_domain(a, b, p):
                out.append(Case("mul8", name, words(a, 8) + words(b, 8), a * b, "b up to 2^256 - 1, a b < 2^256 p"))
    for b in [(1 << 255) - 1, (1 << 255) - (1 << 32)]:                    # a at ITS bound
        a, b = b, (R256 * p - 1) // b
        assert mul8_domain(a, b, p)
        out.append(Case("mul8", name, words(a, 8) + words(b, 8), a * b, "a = 2^255 - 1, a b < 2^256 p"))
    assert all(mul8_domain(val32(c.ins[:8]), val32(c.ins[8:]), p) for c in out)
    return out


# ---------------------------------------------------------------------------------------------------------------- group law
def table_words(pt, p):
    """canonical R'-form affine point as the window table stores it; the identity is (0, 0)"""
    return words(pt[0] * R261 % p, 8) + words(pt[1] * R261 % p, 8)


def abi_words(pt, p):
    return words(pt[0] * R256 % p, 8) + words(pt[1] * R256 % p, 8)


def packed_words(pt, s, p):
    """a packed partial sum (canonical R'-form XYZZ record) of the point with the scale (zz, zzz) = (s^2, s^3); identity: all zero"""
    if pt == (0, 0):
        return [0] * 32
    zz, zzz = s * s % p, s * s * s % p
    return [w for v in (pt[0] * zz, pt[1] * zzz, zz, zzz) for w in words(v * R261 % p, 8)]


def point_of(packed, p):
    """packed R'-form XYZZ record -> the affine point, as integers; checks that the record is canonical and consistent"""
    c = [val32(packed[8 * j: 8 * j + 8]) for j in range(4)]
    assert len(packed) == 32 and all(v < p for v in c)
    ir = pow(R261, -1, p)
    x, y, zz, zzz = [(v * ir) % p for v in c]
    if zz == 0:
        return (0, 0)
    assert (zz * zz * zz - zzz * zzz) % p == 0
    return (x * pow(zz, -1, p) % p, y * pow(zzz, -1, p) % p)


def xyzz_case(cname, p, packed):
    """to_xyzz of a packed record: the same coordinates in the ABI's 2^256 form"""
    ir = pow(R261, -1, p)
    c = [val32(packed[8 * j: 8 * j + 8]) * ir % p for j in range(4)]
    return Case("xyzz", cname, list(packed), [w for v in c for w in words(v * R256 % p, 8)], "packed record")


def predict_chain(cv, init_pt, seq_pts):
    """The sum of a chain (init + entries, each (point, neg)) and whether accumulate_part's fast phase meets an exception on the way: an
    identity entry, an identity running sum, or an entry with the running sum's x (Q = +-acc).  -> (sum, exc, kinds met first)"""
    exc, kind = False, None

    def note(k):
        nonlocal exc, kind
        if not exc:
            exc, kind = True, k
    if init_pt is None:
        (q, n), rest = seq_pts[0], seq_pts[1:]
        acc = cv.neg(q) if n else q
        if q == (0, 0):
            note("first entry O")
    else:
        acc, rest = init_pt, seq_pts
    for q, n in rest:
        if q == (0, 0):
            note("entry O")
        elif acc == (0, 0):
            note("acc O")
        elif acc[0] == q[0]:
            note("Q = acc" if acc == (cv.neg(q) if n else q) else "Q = -acc")
        acc = cv.add(acc, cv.neg(q) if n else q)
    return acc, exc, kind


def plain_sum(cv, seq_pts):
    want = (0, 0)
    for q, n in seq_pts:
        want = cv.add(want, cv.neg(q) if n else q)
    return want


def chain_case(op, cname, cv, seq_pts, init=None, init_pt=None, bound=""):
    """seq_pts: [(affine point, neg)].  chain / chains: want = the sum from the identity.  chainf / chainf_raw: want = (sum with init, exc)."""
    seq = [(table_words(q, cv.p), n) for q, n in seq_pts]
    if op in ("chain", "chains"):
        return Case(op, cname, want=plain_sum(cv, seq_pts), bound=bound, seq=seq)
    total, exc, kind = predict_chain(cv, init_pt if init is not None else None, seq_pts)
    steps = len(seq_pts) - (init is None)
    return Case(op, cname, want=(total, exc, steps), bound=bound + (f" [{kind}]" if exc else ""), seq=seq, init=init)


def check_curve(c, r, p):
    op = c.op
    if op == "tform":
        assert r == c.want, c
    elif op == "xyzz":
        assert r == c.want, c
    elif op in ("chain", "chains", "addp", "dblp"):
        assert point_of(r, p) == c.want, c
    elif op == "chainf":
        total, exc, _ = c.want
        assert len(r) == 33 and r[32] == int(exc), c
        if not exc:
            assert point_of(r[:32], p) == total, c
    elif op == "chainf_raw":
        # curve29.cuh, madd_signed_fast: whatever the operands hold, the result keeps the accumulator's bounds -- x in (P, 9P) normalised,
        # y < 2P normalised (out of mul2), zz, zzz < 2P normalised; before any addition the accumulator is a table entry: x, y <= P.
        total, exc, steps = c.want
        x, y, zz, zzz = (r[9 * i: 9 * i + 9] for i in range(4))
        assert len(r) == 37 and r[36] == int(exc), c
        for l in (x, y, zz, zzz):
            assert all(v < (1 << 29) for v in l[:8]), c
        if steps:
            assert p < val(x) < 9 * p and val(y) < 2 * p and val(zz) < 2 * p and val(zzz) < 2 * p, c
        else:
            assert val(x) < 9 * p and val(y) < 5 * p and val(zz) < 2 * p and val(zzz) < 2 * p, c
        if not exc:
            ir = pow(R261, -1, p)
            X, Y, ZZ, ZZZ = (val(l) * ir % p for l in (x, y, zz, zzz))
            assert ZZ and (ZZ ** 3 - ZZZ ** 2) % p == 0 and (X * pow(ZZ, -1, p) % p, Y * pow(ZZZ, -1, p) % p) == total, c
    else:
        raise AssertionError(op)


def check(c, r):
    """One result against Python integers: congruence, value bound, limb bounds."""
    r = [int(v) for v in r]
    if c.op in ("mul", "mul_ni", "sqr", "sqr_ni", "mul2"):
        check_product(c, r, dict(FIELDS)[c.which])
    elif c.op in ("mul8", "mul8_ni"):
        check_mul8(c, r, dict(FIELDS)[c.which])
    elif c.which in dict(FIELDS):
        check_lazy(c, r, dict(FIELDS)[c.which])
    else:
        check_curve(c, r, P.CURVES[dict(CURVES)[c.which]].p)


def same_record_or_point(a, b, p):
    """The one place where two executors' packed records may differ: `chain` (madd) and `chains` / `chainf` (madd_signed[_fast]) reach the same
    point with another scale of (zz, zzz) when a doubling falls inside the chain -- then the POINTS are compared."""
    return list(a) == list(b) or point_of(a, p) == point_of(b, p)


class GroupCases:
    """The group-law cases of one curve, in two stages: the second (full additions / doublings of packed partial sums, to_xyzz of every record)
    works on the records the first produced on the executor under test."""

    def __init__(self, cname, cid):
        self.cname, self.cv = cname, P.CURVES[cid]
        cv, p = self.cv, self.cv.p
        rnd = random.Random(7 + cid)
        self.pts = pts = [cv.mul(rnd.randrange(1, cv.q), cv.g) for _ in range(12)]
        # plain sums, long enough for the lazy bounds to reach their steady state
        self.seqs = [("40 additions", [(rnd.choice(pts), rnd.random() < 0.5) for _ in range(40)])]
        # exceptional cases inside a chain: first addition onto the identity, Q = acc (doubling), Q = -acc (back to the identity),
        # identity table entries (skipped bases), and again after the identity
        A, B = pts[0], pts[1]
        O = (0, 0)
        self.seqs += [("exceptional", s) for s in [
            [(A, False)], [(A, False), (A, False)], [(A, False), (A, True)], [(A, False), (A, True), (B, False)],
            [(O, False)], [(A, False), (O, False), (B, True)], [(A, False), (A, False), (A, False), (A, False)],
            [(A, False), (B, False), (cv.add(A, B), True)], [(A, False), (B, False), (cv.add(A, B), False)]]]
        # operands of the full additions
        self.named = {"S1": [(pts[2], False), (pts[3], False), (pts[4], True)], "S2": [(pts[5], False), (pts[6], True)],
                      "Z": [(A, False), (A, True)], "S1n": [(pts[2], True), (pts[3], True), (pts[4], False)]}
        self.seqs += [(k, v) for k, v in self.named.items()]
        # ---- the chain as accumulate_part runs it
        S = cv.add(cv.add(pts[7], pts[8]), cv.neg(pts[9]))
        scale = rnd.randrange(2, p)
        inits = {"sum": (S, packed_words(S, scale, p)), "A scaled": (A, packed_words(A, scale, p)), "A": (A, packed_words(A, 1, p)),
                 "O": (O, [0] * 32), "O, x y left over": (O, words(5, 8) + words(7, 8) + [0] * 16)}
        self.fast = []                                     # (label, init name or None, sequence)
        for label, s in self.seqs:
            self.fast.append((label, None, s))
        tail = [(pts[10], False), (pts[11], True)]
        for s in ([(B, False)], [(B, False), (pts[2], True), (pts[3], False)], self.seqs[0][1]):
            self.fast.append(("init sum", "sum", s))
        for iname in ("A scaled", "A"):
            self.fast += [("init = Q", iname, [(A, False)]), ("init = -Q", iname, [(A, True)]), ("init = Q later", iname, [(B, False), (B, True), (A, False)]),
                          ("init, no exception", iname, [(B, False), (pts[2], True)])]
        for iname in ("O", "O, x y left over"):            # a partial sum that cancelled to the identity (the r06 slot-mode case)
            self.fast += [("init O", iname, [(A, False)]), ("init O", iname, [(A, True), (B, False), (pts[2], False)])]
        self.fast += [("init, entry O", "sum", [(O, False)]), ("init, entry O", "sum", [(B, False), (O, True), (A, False)]),
                      ("sum back to O", "sum", [(pts[9], False), (pts[8], True), (pts[7], True), (B, False)]),
                      ("sum back to O exactly at the end", "sum", [(pts[9], False), (pts[8], True), (pts[7], True)])]
        self.inits, self.tail = inits, tail

    def tform_cases(self):
        """table_form of every point a sequence uses (ABI affine -> the table's R'-form)"""
        p = self.cv.p
        used = [q for _, s in self.seqs for q, _ in s] + self.pts + [(0, 0)]
        return [Case("tform", self.cname, abi_words(q, p), table_words(q, p), "point" if q != (0, 0) else "identity") for q in used]

    def chain_cases(self, op):
        return [chain_case(op, self.cname, self.cv, s, bound=label) for label, s in self.seqs]

    def chainf_cases(self, op="chainf"):
        out = []
        for label, iname, s in self.fast:
            ipt, iw = self.inits[iname] if iname else (None, None)
            out.append(chain_case(op, self.cname, self.cv, s, init=iw, init_pt=ipt, bound=label))
            if op == "chainf_raw":                         # and one, two further additions on top of whatever the chain left
                for more in (1, 2):
                    out.append(chain_case(op, self.cname, self.cv, s + self.tail[:more], init=iw, init_pt=ipt, bound=label + f" + {more} more"))
        return out

    def stage2(self, records):
        """records: {label of self.seqs: packed record of `chains`} from the executor -> addp / dblp / xyzz cases"""
        cv, name = self.cv, self.cname
        p = cv.p
        rec = {k: list(records[k]) for k in self.named}
        pt = {k: point_of(v, p) for k, v in rec.items()}
        S1, S2, Z, S1n = rec["S1"], rec["S2"], rec["Z"], rec["S1n"]
        add = lambda a, b, want, bound: Case("addp", name, a + b, want, bound)
        out = [add(S1, S2, cv.add(pt["S1"], pt["S2"]), "a + b"), add(S1, S1, cv.add(pt["S1"], pt["S1"]), "equal operands -> doubling"),
               add(S1, S1n, (0, 0), "opposite operands"), add(Z, S2, pt["S2"], "O + b"), add(S2, Z, pt["S2"], "a + O"), add(Z, Z, (0, 0), "O + O"),
               Case("dblp", name, S1, cv.add(pt["S1"], pt["S1"]), "2 a"), Case("dblp", name, Z, (0, 0), "2 O")]
        return out


# ------------------------------------------------------------------------------------------------------- random chains (device)
def random_chain_cases(cname, cid, count=4096, seed=64):
    """Chains of 1 .. 64 additions over a pool of 12 points, their negatives and the identity entry, with repetition, so that Q = acc,
    Q = -acc, identity entries and "back to the identity, then more" fall at random positions; every second one starts from a packed
    partial sum (`init`), some of those the identity.  -> {"chain" | "chains": the entries from the identity, "chainf": with init}, and
    how many chains met which exception first.  Asserts that the set is neither free of exceptions nor made of them: 20 % .. 80 % of the
    chains are exceptional, and every kind of exception occurs."""
    cv = P.CURVES[cid]
    p = cv.p
    rnd = random.Random(seed + cid)
    pool = [cv.mul(rnd.randrange(1, cv.q), cv.g) for _ in range(12)]
    O = (0, 0)
    tw = {q: table_words(q, p) for q in pool + [O]}
    out, kinds = {"chain": [], "chains": [], "chainf": []}, {}
    for s in range(count):
        n = rnd.randint(1, 64) if rnd.random() < 0.5 else rnd.randint(1, 8)      # half of them short: the start of a chain is where a small pool collides
        pts = []
        for _ in range(n):
            u = rnd.random()
            if u < 0.01:
                pts.append((O, rnd.random() < 0.5))
            elif u < 0.06 and pts:
                pts.append((rnd.choice(pts)[0], rnd.random() < 0.5))                # an entry again: Q = +-acc after a cancellation
            else:
                pts.append((rnd.choice(pool), rnd.random() < 0.5))
        init = ipt = None
        if s & 1:
            if rnd.random() < 0.1:
                ipt = O
            else:
                ipt = plain_sum(cv, [(rnd.choice(pool), rnd.random() < 0.5) for _ in range(rnd.randint(1, 3))])
            init = packed_words(ipt, rnd.randrange(1, p), p)
        total, exc, kind = predict_chain(cv, ipt, pts)
        kinds[kind] = kinds.get(kind, 0) + 1
        seq = [(tw[q], neg) for q, neg in pts]
        plain = total if ipt is None else cv.add(total, cv.neg(ipt))
        out["chain"].append(Case("chain", cname, want=plain, bound=f"random chain {s}", seq=seq))
        out["chains"].append(Case("chains", cname, want=plain, bound=f"random chain {s}", seq=seq))
        out["chainf"].append(Case("chainf", cname, want=(total, exc, n - (init is None)), bound=f"random chain {s}" + (f" [{kind}]" if exc else ""),
                                  seq=seq, init=init))
    share = 1 - kinds.get(None, 0) / count
    assert 0.2 <= share <= 0.8, (share, kinds)
    assert all(kinds.get(k, 0) >= count // 128 for k in ("entry O", "acc O", "Q = acc", "Q = -acc")), kinds
    return out, kinds


# ------------------------------------------------------------------------------------------------------------ bulk layer (device)
def bulk_value(p, rnd, kmax):
    """k p + {0, 1, p - 1, p / 2, random} below kmax p: the bound-hugging mixture of edge_values, drawn"""
    k = rnd.randrange(kmax)
    u = rnd.randrange(8)
    return k * p + (0, 1, p - 1, p // 2)[u] if u < 4 else k * p + rnd.randrange(p)


def bulk_cases(op, name, p, count, seed):
    """`count` seeded cases of one operation drawn inside its stated bounds (values from bulk_value, limbs re-distributed at random up
    to the admissible width).  The same Case objects as the edge cases: `check` judges them."""
    rnd = random.Random(seed)
    out = []
    for i in range(count):
        if op in ("mul", "mul_ni"):
            a, b = bulk_value(p, rnd, 13), bulk_value(p, rnd, 12)
            wa, wb = rnd.choice(((2, 0), (2, 0), (1, 1), (0, 0)))
            la, lb = limbs29(a, wa, rnd), limbs29(b, wb, rnd)
            out.append(Case(op, name, la + lb, a * b, "bulk"))
        elif op in ("sqr", "sqr_ni"):
            a = bulk_value(p, rnd, 13)
            out.append(Case(op, name, limbs29(a, rnd.randrange(2), rnd), a * a, "bulk"))
        elif op == "mul2":
            a, b, c, d = bulk_value(p, rnd, 12), bulk_value(p, rnd, 8), bulk_value(p, rnd, 6), bulk_value(p, rnd, 2)
            out.append(Case(op, name, limbs29(a, rnd.randrange(2), rnd) + limbs29(b) + limbs29(c, rnd.randrange(2), rnd) + limbs29(d), a * b + c * d, "bulk"))
        elif op == "norm":
            a = bulk_value(p, rnd, 13)
            out.append(Case(op, name, limbs29(a, 2, rnd), a, "bulk"))
        elif op == "add":
            a, b = bulk_value(p, rnd, 13), bulk_value(p, rnd, 13)
            out.append(Case(op, name, limbs29(a, 2, rnd) + limbs29(b, 2, rnd), a + b, "bulk"))
        elif op in ("sub", "neg"):
            cp, e = SUB_PAIRS[i % len(SUB_PAIRS)]
            while True:
                b = bulk_value(p, rnd, cp)
                lb = limbs29(b, e, rnd)
                if lb[8] <= ((cp * p) >> 232) - (1 << e):
                    break
            a = bulk_value(p, rnd, 13)
            if op == "sub":
                out.append(Case(op, name, limbs29(a, 1, rnd) + lb, a - b + cp * p, "bulk", cp, e))
            else:
                out.append(Case(op, name, lb, cp * p - b, "bulk", cp, e))
        elif op == "canon":
            v = bulk_value(p, rnd, 4)
            out.append(Case(op, name, limbs29(v), v % p, "bulk"))
        elif op == "redlazy":
            v = min(bulk_value(p, rnd, 677), (1 << 263) - 1) if rnd.random() < 0.7 else rnd.randrange(1 << 263)
            out.append(Case(op, name, limbs29(v), v, "bulk"))
        elif op in ("unpack", "pack"):
            v = rnd.choice((bulk_value(p, rnd, 5), rnd.randrange(R256), R256 - 1 - rnd.randrange(1 << 32)))
            v = min(v, R256 - 1)
            out.append(Case(op, name, words(v, 8) if op == "unpack" else limbs29(v), v, "bulk"))
        elif op in ("mul8", "mul8_ni"):
            a, b = bulk_value(p, rnd, 1), bulk_value(p, rnd, 1)
            u = rnd.randrange(8)
            if u == 0:
                a, b = bulk_value(p, rnd, 2), bulk_value(p, rnd, 2)
            elif u == 1:
                b = rnd.randrange(R256)
                a = rnd.randrange(min(p, (R256 * p - 1) // max(b, 1) + 1))
            assert mul8_domain(a, b, p)
            out.append(Case(op, name, words(a, 8) + words(b, 8), a * b, "bulk"))
        else:
            raise AssertionError(op)
    return out


def counts(cases):
    n = {}
    for c in cases:
        n[c.op] = n.get(c.op, 0) + 1
    return n
