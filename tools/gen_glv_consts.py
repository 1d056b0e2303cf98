"""Generates sirius_amd/csrc/glv_consts.inc: the constants of the endomorphism split used by compact commitment keys.

bn256 G1 (y^2 = x^3 + 3 over Fq, order r) and grumpkin (y^2 = x^3 - 17 over Fr, order q) have j-invariant 0:
phi(x, y) = (beta x, y) is the multiplication by lambda, with beta / lambda cube roots of unity of the base / scalar field.
A scalar k splits as k = k1 + lambda k2 (mod n) with |k1|, |k2| < 2^127, so windows 8..15 of 2^(16 w) P are
phi of windows 0..7 and a key needs to store only eight of them (msm.hip, glv.cuh).

Everything below follows from the two moduli and the curve equations; nothing is typed in.  Per curve:
  lambda, beta     canonical integers; beta is the root with [lambda] G = (beta Gx, Gy), checked here on the generator
  (a1, b1), (a2, b2)   reduced basis of the lattice {(x, y): x + lambda y = 0 mod n}  (extended Euclid, as in GLV 2001)
  g1, g2, SH1, SH2     fixed-point reciprocals: c1 = (k g1 + 2^(SH1-1)) >> SH1 ~ round(k |b2| / n), c2 likewise from |b1|
  A1, A2, B1, B2       signed multipliers: k1 = k + c1 A1 + c2 A2,  k2 = c1 B1 + c2 B2
  beta29               beta in the R' = 2^261 Montgomery form of the 9 x 29-bit multiplier (field29.cuh)
The size bound is PROVEN for the emitted rounding, not sampled: see prove_bound()."""
import math
import os
import sys
from fractions import Fraction

FR = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001      # bn256 scalar field = grumpkin base field
FQ = 0x30644e72e131a029b85045b68181585d97816a916871ca8d3c208c16d87cfd47      # bn256 base field = grumpkin scalar field
GW = 160            # bits of a fixed-point reciprocal (5 words: the quotient is the high part of a 256 x 160-bit product)
SH_MAX = 288        # 128 quotient bits are read from bit SH of the 416-bit product
KBITS = 127         # |k1|, |k2| < 2^KBITS: the top signed 16-bit digit of a half never carries out


def sqrt_mod(a, p):
    """Tonelli-Shanks; the smaller root."""
    a %= p
    if a == 0:
        return 0
    assert pow(a, (p - 1) // 2, p) == 1
    s, t = p - 1, 0
    while s % 2 == 0:
        s //= 2
        t += 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, u, r = t, pow(z, s, p), pow(a, s, p), pow(a, (s + 1) // 2, p)
    while u != 1:
        i, v = 0, u
        while v != 1:
            v = v * v % p
            i += 1
        b = pow(c, 1 << (m - i - 1), p)
        m, c = i, b * b % p
        u, r = u * c % p, r * b % p
    return min(r, p - r)


# (name, base field, scalar field, b of y^2 = x^3 + b, generator) -- curve ids as in include/sirius_amd.h
CURVES = [("bn256 G1", FQ, FR, 3, (1, 2)),
          ("grumpkin", FR, FQ, -17, (1, sqrt_mod(-16, FR)))]


def cube_root_of_unity(n):
    """The smaller of the two non-trivial cube roots of unity mod n."""
    g = 2
    while pow(g, (n - 1) // 3, n) == 1:
        g += 1
    w = pow(g, (n - 1) // 3, n)
    return min(w, w * w % n)


def ec_add(P, Q, p):
    if P is None:
        return Q
    if Q is None:
        return P
    (x1, y1), (x2, y2) = P, Q
    if x1 == x2:
        if (y1 + y2) % p == 0:
            return None
        m = 3 * x1 * x1 * pow(2 * y1, -1, p) % p
    else:
        m = (y2 - y1) * pow(x2 - x1, -1, p) % p
    x3 = (m * m - x1 - x2) % p
    return x3, (m * (x1 - x3) - y1) % p


def ec_mul(k, P, p):
    acc = None
    while k:
        if k & 1:
            acc = ec_add(acc, P, p)
        P = ec_add(P, P, p)
        k >>= 1
    return acc


def lattice_basis(n, lam):
    rs, ts = [n, lam], [0, 1]
    while rs[-1]:
        q = rs[-2] // rs[-1]
        rs.append(rs[-2] - q * rs[-1])
        ts.append(ts[-2] - q * ts[-1])
    root = math.isqrt(n)
    l = max(i for i in range(len(rs)) if rs[i] >= root)
    v1 = (rs[l + 1], -ts[l + 1])
    v2 = min((rs[l], -ts[l]), (rs[l + 2], -ts[l + 2]), key=lambda v: v[0] * v[0] + v[1] * v[1])
    return v1, v2


def derive(p, n, b, G):
    assert (G[1] * G[1] - G[0] ** 3 - b) % p == 0 and ec_mul(n, G, p) is None
    lam = cube_root_of_unity(n)
    assert lam != 1 and pow(lam, 3, n) == 1
    lG = ec_mul(lam, G, p)
    w = cube_root_of_unity(p)
    beta = [c for c in (w, w * w % p) if (c * G[0] % p, G[1]) == lG]
    assert len(beta) == 1, "no cube root of unity of the base field matches lambda"
    beta = beta[0]
    (a1, b1), (a2, b2) = lattice_basis(n, lam)
    assert (a1 + lam * b1) % n == 0 and (a2 + lam * b2) % n == 0
    D = a1 * b2 - a2 * b1
    assert abs(D) == n
    # (k, 0) = x1 v1 + x2 v2 with x1 = k b2 / D, x2 = -k b1 / D; c1 = round(k |b2| / n) >= 0 carries the sign s1 of b2 / D, c2 that of -b1 / D
    s1 = 1 if (b2 > 0) == (D > 0) else -1
    s2 = 1 if (-b1 > 0) == (D > 0) else -1
    sh1 = min(SH_MAX, max(s for s in range(254, 512) if (abs(b2) << s) // n < 1 << GW))
    sh2 = min(SH_MAX, max(s for s in range(254, 512) if (abs(b1) << s) // n < 1 << GW))
    c = dict(p=p, n=n, lam=lam, beta=beta, a1=a1, b1=b1, a2=a2, b2=b2, sh1=sh1, sh2=sh2, g1=(abs(b2) << sh1) // n, g2=(abs(b1) << sh2) // n,
             A1=-s1 * a1, A2=-s2 * a2, B1=-s1 * b1, B2=-s2 * b2)
    prove_bound(c)
    return c


def prove_bound(c):
    """|k1|, |k2| < 2^KBITS for EVERY 0 <= k < n under the emitted rounding.
    c_i = floor(k g_i / 2^SH + 1/2) with g_i = floor(2^SH |b| / n):  k |b| / n - k / 2^SH < k g_i / 2^SH <= k |b| / n, and k < n, so
    |c_i - x_i| <= 1/2 + n / 2^SH =: e_i  (x_i the exact rational coordinate).  (k1, k2) = (x1 - c1) v1 + (x2 - c2) v2, hence
    |k1| <= e1 |a1| + e2 |a2| and |k2| <= e1 |b1| + e2 |b2|."""
    n = c["n"]
    e1 = Fraction(1, 2) + Fraction(n, 1 << c["sh1"])
    e2 = Fraction(1, 2) + Fraction(n, 1 << c["sh2"])
    k1_max = e1 * abs(c["a1"]) + e2 * abs(c["a2"])
    k2_max = e1 * abs(c["b1"]) + e2 * abs(c["b2"])
    assert k1_max < 1 << KBITS and k2_max < 1 << KBITS, "the rounding scheme does not keep |k1|, |k2| below 2^%d" % KBITS
    assert c["g1"] < 1 << GW and c["g2"] < 1 << GW and c["sh1"] + 128 <= 32 * 13 and c["sh2"] + 128 <= 32 * 13
    # the quotients (<= |b| + 1) and the multipliers fit 128 bits; the body adds their products modulo 2^256, which is exact for a
    # result below 2^KBITS in magnitude whatever the partial sums do
    assert max(abs(c["b1"]), abs(c["b2"])) + 2 < 1 << 128 and all(abs(c[x]) < 1 << 128 for x in ("A1", "A2", "B1", "B2"))
    c["k1_max"], c["k2_max"] = int(k1_max), int(k2_max)


def decompose(c, k):
    """The emitted scheme in integers (what glv.cuh computes); returns signed (k1, k2)."""
    c1 = (k * c["g1"] + (1 << (c["sh1"] - 1))) >> c["sh1"]
    c2 = (k * c["g2"] + (1 << (c["sh2"] - 1))) >> c["sh2"]
    return k + c1 * c["A1"] + c2 * c["A2"], c1 * c["B1"] + c2 * c["B2"]


def words(x, count, bits=32):
    assert 0 <= x < 1 << (count * bits) or (bits == 29 and 0 <= x < 1 << 261)
    return [(x >> (bits * i)) & ((1 << bits) - 1) for i in range(count)]


def emit_fn(w, name, vals, note):
    w(f"    SRS_HD static constexpr uint32_t {name}(int i) {{   // {note}")
    w(f"        constexpr uint32_t m[{len(vals)}] = {{" + ", ".join(f"0x{v:08x}u" for v in vals) + "};")
    w("        return m[i];")
    w("    }")


def main():
    out = []
    w = out.append
    w("// GENERATED by tools/gen_glv_consts.py -- do not edit.  Constants of the endomorphism split (glv.cuh); little-endian 32-bit words")
    w("// unless stated.  The generator proves |k1|, |k2| < 2^%d for every scalar below the group order." % KBITS)
    w("template <int CURVE> struct GlvConsts;")
    for cid, (name, p, n, b, G) in enumerate(CURVES):
        c = derive(p, n, b, G)
        for k in (0, 1, 2, n - 1, n - 2, c["lam"], c["lam"] + 1, c["lam"] - 1, (1 << 128) - 1, 1 << 253, (n - 1) // 2):
            k1, k2 = decompose(c, k)
            assert (k1 + c["lam"] * k2 - k) % n == 0 and abs(k1) <= c["k1_max"] and abs(k2) <= c["k2_max"]
        w(f"// {name}: lambda = 0x{c['lam']:x}")
        w(f"//   beta = 0x{c['beta']:x}")
        w(f"//   basis ({c['a1']}, {c['b1']}), ({c['a2']}, {c['b2']})")
        w(f"//   proven: |k1| <= 0x{c['k1_max']:x}, |k2| <= 0x{c['k2_max']:x}")
        w(f"template <> struct GlvConsts<{cid}> {{")
        emit_fn(w, "lambda", words(c["lam"], 8), "cube root of unity of the scalar field")
        emit_fn(w, "beta", words(c["beta"], 8), "cube root of unity of the base field: (beta x, y) = [lambda](x, y)")
        emit_fn(w, "beta29", words(c["beta"] * (1 << 261) % p, 9, 29), "beta 2^261 mod p, 9 x 29-bit limbs")
        emit_fn(w, "g1", words(c["g1"], GW // 32), "floor(2^SH1 |b2| / n)")
        emit_fn(w, "g2", words(c["g2"], GW // 32), "floor(2^SH2 |b1| / n)")
        for nm in ("A1", "A2", "B1", "B2"):
            emit_fn(w, nm.lower(), words(abs(c[nm]), 4), f"|{nm}|")
        w(f"    static constexpr int SH1 = {c['sh1']}, SH2 = {c['sh2']};")
        w("    static constexpr bool " + ", ".join(f"NEG_{nm} = {'true' if c[nm] < 0 else 'false'}" for nm in ("A1", "A2", "B1", "B2")) + ";")
        w("};")
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "sirius_amd", "csrc", "glv_consts.inc")
    if len(sys.argv) > 1:          # another place (tests/test_glv_host.py compares it with the committed file)
        path = sys.argv[1]
    with open(path, "w") as f:
        f.write("\n".join(out) + "\n")
    print("wrote", os.path.normpath(path))


if __name__ == "__main__":
    main()
