// glv.cuh -- the endomorphism split of a scalar, for compact commitment keys (msm.hip).
//
// bn256 G1 and grumpkin have j-invariant 0: phi(x, y) = (beta x, y) = [lambda](x, y).  A scalar k < n is written
// k = k1 + lambda k2 (mod n) with |k1|, |k2| < 2^127 (GLV 2001: Babai rounding against a reduced basis of the lattice
// {(x, y): x + lambda y = 0 mod n}), so  k P = k1 P + k2 phi(P):  the eight upper 16-bit windows of k P become the eight lower
// windows of phi(P), and phi costs one field product on x.
// Plain integer C++, host and device: srs_glv_decompose (capi.hip) runs this very body without a device.  Constants and the
// proof of the size bound: tools/gen_glv_consts.py -> glv_consts.inc.
#pragma once
#include "curve.cuh"

namespace srs {

#include "glv_consts.inc"

struct glv_t {
    uint32_t k1[4], k2[4];   // |k1|, |k2| < 2^127
    bool neg1, neg2;         // k1 < 0, k2 < 0
};

namespace glv_detail {

// word i of the curve's constant number W: the two reciprocals, then the four multipliers (folds to a literal after unrolling)
template <class K, int W>
SRS_HD constexpr uint32_t word(int i) {
    return W == 0 ? K::g1(i) : W == 1 ? K::g2(i) : W == 2 ? K::a1(i) : W == 3 ? K::a2(i) : W == 4 ? K::b1(i) : K::b2(i);
}

// (k g + 2^(SH - 1)) >> SH for k < 2^256, g < 2^160 (constant W): the rounded quotient, 128 bits
template <class K, int W, int SH>
SRS_HD void rounded_quotient(const fe_t &k, uint32_t (&c)[4]) {
    uint32_t prod[13];
#pragma unroll
    for (int i = 0; i < 13; ++i) prod[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint32_t carry = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint64_t t = (uint64_t)k.v[i] * word<K, W>(j) + prod[i + j] + carry;
            prod[i + j] = (uint32_t)t;
            carry = (uint32_t)(t >> 32);
        }
        prod[i + 5] = carry;
    }
    {   // + 2^(SH - 1): round to nearest
        constexpr int L = (SH - 1) / 32;
        uint64_t t = (uint64_t)prod[L] + (1u << ((SH - 1) % 32));
        prod[L] = (uint32_t)t;
#pragma unroll
        for (int i = L + 1; i < 13; ++i) {
            t = (uint64_t)prod[i] + (t >> 32);
            prod[i] = (uint32_t)t;
        }
    }
    constexpr int L = SH / 32, S = SH % 32;
    static_assert(L + 3 < 13 && (S == 0 || L + 4 < 13), "the quotient's 128 bits lie inside the product");
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t x = prod[L + j] >> S;
        if (S != 0) x |= prod[L + j + 1] << ((32 - S) % 32);
        c[j] = x;
    }
}

// acc (256 bits, two's complement) +- c * m, c and m (constant W) < 2^128
template <class K, int W, bool NEG>
SRS_HD void mul_acc(uint32_t (&acc)[8], const uint32_t (&c)[4]) {
    uint32_t prod[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) prod[i] = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t carry = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint64_t t = (uint64_t)c[i] * word<K, W>(j) + prod[i + j] + carry;
            prod[i + j] = (uint32_t)t;
            carry = (uint32_t)(t >> 32);
        }
        prod[i + 4] = carry;
    }
    if (NEG) {
        uint32_t borrow = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t t = (uint64_t)acc[i] - prod[i] - borrow;
            acc[i] = (uint32_t)t;
            borrow = (uint32_t)(t >> 32) & 1u;
        }
    } else {
        uint32_t carry = 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint64_t t = (uint64_t)acc[i] + prod[i] + carry;
            acc[i] = (uint32_t)t;
            carry = (uint32_t)(t >> 32);
        }
    }
}

// two's complement 256-bit value of magnitude < 2^127 -> magnitude and sign
SRS_HD bool split_sign(const uint32_t (&v)[8], uint32_t (&mag)[4]) {
    const bool neg = (v[7] >> 31) != 0;
    uint32_t carry = neg ? 1u : 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t t = (uint64_t)(neg ? ~v[i] : v[i]) + carry;
        mag[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
    return neg;
}

}  // namespace glv_detail

// k: canonical scalar of curve C (below the group order)
template <class C>
SRS_HD glv_t glv_decompose(const fe_t &k) {
    using K = GlvConsts<C::ID>;
    uint32_t c1[4], c2[4];
    glv_detail::rounded_quotient<K, 0, K::SH1>(k, c1);
    glv_detail::rounded_quotient<K, 1, K::SH2>(k, c2);
    uint32_t k1[8], k2[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        k1[i] = k.v[i];
        k2[i] = 0;
    }
    glv_detail::mul_acc<K, 2, K::NEG_A1>(k1, c1);      // k1 = k + c1 A1 + c2 A2
    glv_detail::mul_acc<K, 3, K::NEG_A2>(k1, c2);
    glv_detail::mul_acc<K, 4, K::NEG_B1>(k2, c1);      // k2 = c1 B1 + c2 B2
    glv_detail::mul_acc<K, 5, K::NEG_B2>(k2, c2);
    glv_t o;
    o.neg1 = glv_detail::split_sign(k1, o.k1);
    o.neg2 = glv_detail::split_sign(k2, o.k2);
    return o;
}

}  // namespace srs
