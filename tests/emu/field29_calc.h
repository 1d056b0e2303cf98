// field29_calc.h -- TEST INFRASTRUCTURE shared by the two calculators of the lazy 9 x 29-bit arithmetic: tests/emu/field29_check.cpp
// (host build of the headers' C++ bodies) and tests/devcalc/devcalc.hip (the generated device bodies in kernels of their own).  What both
// must agree on lives here once, so that the two cannot drift:
//   * the (CP, E) instantiations of Fp29::sub_lazy / neg_lazy that can be asked for;
//   * the chain of gathered mixed additions as the bucket accumulation runs it (`chainf`).
#pragma once
#include "curve29.cuh"

// every (CP, E) pair curve29.cuh, the sweep emitter and the NTT tile use (tests/field29_cases.py: SUB_PAIRS is the same list)
#define SRS_CALC_SUB_PAIRS(X) \
    X(1, 0) X(2, 0) X(3, 0) X(5, 1) X(6, 2) X(7, 2) X(8, 0) X(10, 0) X(13, 0) X(31, 0) X(3, 2) X(12, 2) X(6, 0) X(8, 1)

namespace srs {

// One table entry of a chain as both calculators take it: 16 words (x, y of a canonical R'-form affine point) and a sign word.
static constexpr unsigned CALC_ENTRY_WORDS = 17;

SRS_HD affine_t calc_entry(const uint32_t *w) {
    affine_t q;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        q.x.v[i] = w[i];
        q.y.v[i] = w[8 + i];
    }
    return q;
}

// The first phase of accumulate_part (csrc/msm.hip:1236-1279; that function is a template inside msm.hip and cannot be included), without
// its software prefetch of the gathered points: init (nullptr: a fresh part, whose first entry IS the sum so far and is flagged when it is
// the table's identity) + the n >= 1 entries, every further one through Ec29::madd_signed_fast with ONE sticky flag.  The second phase -- the
// whole chain once more through madd_signed when the flag is set -- is the calculators' `chains`.
template <class C>
SRS_HD xyzz29_t calc_chainf(const xyzz_t *init, unsigned n, const uint32_t *entries, bool &exc) {
    using E29 = Ec29<C>;
    using F = typename E29::F;
    exc = false;
    xyzz29_t acc;
    unsigned j = 0;
    if (init) {
        acc = E29::unpack(*init);
    } else {
        const aff29_t q = E29::load_raw(calc_entry(entries));
        acc.x = q.x;
        acc.y = entries[16] ? F::normalize(F::template neg_lazy<1, 0>(q.y)) : q.y;      // msm.hip:1258
        acc.zz = E29::one();
        acc.zzz = acc.zz;
        exc = F::is_zero_exact(q.y);                                                     // msm.hip:1261
        j = 1;
    }
    for (; j < n; ++j) {
        const uint32_t *w = entries + (size_t)j * CALC_ENTRY_WORDS;
        acc = E29::madd_signed_fast(acc, E29::load_raw(calc_entry(w)), w[16] != 0, exc);  // msm.hip:1274
    }
    return acc;
}

}  // namespace srs
