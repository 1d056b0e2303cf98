// devcalc.hip -- TEST INFRASTRUCTURE, never linked into libsirius_amd.so.  The device twin of tests/emu/field29_check.cpp: the same
// operations of field29.cuh / curve29.cuh / field.cuh, but compiled by hipcc for the GPU, where Fp29::mul / mul2 / sqr are the generated
// chained bodies (field29_chain.inc) and Fp::mul is the generated FIPS body (field_fips.inc) -- the code the product's kernels run, which
// no host build can execute.  tests/test_field29_gpu.py feeds both calculators the vectors of tests/field29_cases.py.
//
// One kernel per operation, one thread per case, 256-thread workgroups; operands and results are flat uint32_t arrays, `in_words` /
// `out_words` per case, in the word order the host calculator reads and prints.  Plain C++ on the product's headers: no tuning, no
// streams, no state, no assembly of its own.
#define SRS_F29_CHAIN 1          // exactly as csrc/msm.hip and csrc/ntt.hip select the chained bodies
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "field29_calc.h"

// field29.cuh takes the generated bodies under `defined(SRS_F29_CHAIN) && defined(__HIP_DEVICE_COMPILE__)`; a device pass without the
// macro would silently compile the C++ twin -- the code tests/emu/field29_check.cpp already covers -- and make this calculator pointless.
// (What the binary holds is checked as well: tests/test_field29_devcalc_build.py counts the multiply-accumulates of the Fr `mul` kernel.)
#if defined(__HIP_DEVICE_COMPILE__) && !defined(SRS_F29_CHAIN)
#error "devcalc: the chained device bodies of Fp29 (field29_chain.inc) are not the ones in effect"
#endif

using namespace srs;

namespace {

enum Op : int {
    OP_MUL = 0, OP_MUL_NI, OP_SQR, OP_SQR_NI, OP_MUL2, OP_NORM, OP_ADD, OP_CANON, OP_REDLAZY, OP_UNPACK, OP_PACK, OP_MUL8, OP_MUL8_NI,
    OP_CHAIN, OP_CHAINS, OP_CHAINF, OP_CHAINF_RAW, OP_ADDP, OP_DBLP, OP_TFORM, OP_XYZZ, OP_SUB, OP_NEG
};

// the called form (cf. mul_ni / mul29_ni in csrc/rowprog_dev.cuh): operands and result travel through the calling convention
template <class P>
__device__ __attribute__((noinline)) f29_t mul29_called(f29_t a, f29_t b) { return Fp29<P>::mul(a, b); }
template <class P>
__device__ __attribute__((noinline)) f29_t sqr29_called(f29_t a) { return Fp29<P>::sqr(a); }
template <class P>
__device__ __attribute__((noinline)) fe_t mul8_called(fe_t a, fe_t b) { return Fp<P>::mul(a, b); }

__device__ __forceinline__ f29_t ld9(const uint32_t *w) {
    f29_t a;
#pragma unroll
    for (int i = 0; i < 9; ++i) a.v[i] = w[i];
    return a;
}
__device__ __forceinline__ fe_t ld8(const uint32_t *w) {
    fe_t a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a.v[i] = w[i];
    return a;
}
__device__ __forceinline__ xyzz_t ld32(const uint32_t *w) {
    xyzz_t p;
    p.x = ld8(w);
    p.y = ld8(w + 8);
    p.zz = ld8(w + 16);
    p.zzz = ld8(w + 24);
    return p;
}
__device__ __forceinline__ void st9(uint32_t *w, const f29_t &a) {
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = a.v[i];
}
__device__ __forceinline__ void st8(uint32_t *w, const fe_t &a) {
#pragma unroll
    for (int i = 0; i < 8; ++i) w[i] = a.v[i];
}
__device__ __forceinline__ void st32(uint32_t *w, const xyzz_t &p) {
    st8(w, p.x);
    st8(w + 8, p.y);
    st8(w + 16, p.zz);
    st8(w + 24, p.zzz);
}

template <class P, int OP>
__global__ void __launch_bounds__(256) k_field(uint32_t n, const uint32_t *__restrict__ in, uint32_t wi, uint32_t *__restrict__ out, uint32_t wo) {
    using G = Fp29<P>;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const uint32_t *c = in + (size_t)i * wi;
        uint32_t *o = out + (size_t)i * wo;
        if constexpr (OP == OP_MUL) st9(o, G::mul(ld9(c), ld9(c + 9)));
        else if constexpr (OP == OP_MUL_NI) st9(o, mul29_called<P>(ld9(c), ld9(c + 9)));
        else if constexpr (OP == OP_SQR) st9(o, G::sqr(ld9(c)));
        else if constexpr (OP == OP_SQR_NI) st9(o, sqr29_called<P>(ld9(c)));
        else if constexpr (OP == OP_MUL2) st9(o, G::mul2(ld9(c), ld9(c + 9), ld9(c + 18), ld9(c + 27)));
        else if constexpr (OP == OP_NORM) st9(o, G::normalize(ld9(c)));
        else if constexpr (OP == OP_ADD) st9(o, G::add_lazy(ld9(c), ld9(c + 9)));
        else if constexpr (OP == OP_CANON) st8(o, G::to_canonical_fe(ld9(c)));
        else if constexpr (OP == OP_REDLAZY) st9(o, G::reduce_lazy(ld9(c)));
        else if constexpr (OP == OP_UNPACK) st9(o, G::unpack(ld8(c)));
        else if constexpr (OP == OP_PACK) st8(o, G::pack(ld9(c)));
        else if constexpr (OP == OP_MUL8) st8(o, Fp<P>::mul(ld8(c), ld8(c + 8)));
        else if constexpr (OP == OP_MUL8_NI) st8(o, mul8_called<P>(ld8(c), ld8(c + 8)));
    }
}

template <class P, uint32_t CP, uint32_t E, bool NEG>
__global__ void __launch_bounds__(256) k_sub(uint32_t n, const uint32_t *__restrict__ in, uint32_t wi, uint32_t *__restrict__ out, uint32_t wo) {
    using G = Fp29<P>;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const uint32_t *c = in + (size_t)i * wi;
        uint32_t *o = out + (size_t)i * wo;
        if constexpr (NEG) st9(o, G::template neg_lazy<CP, E>(ld9(c)));
        else st9(o, G::template sub_lazy<CP, E>(ld9(c), ld9(c + 9)));
    }
}

// chain / chains: n (w[16] neg){n}            chainf / chainf_raw: has_init init[32] n (w[16] neg){n}   (init always present, ignored without has_init)
// The entry count is clamped to what the case's `wi` words hold, so a wrong header word cannot read outside the case.
template <class C, int OP>
__global__ void __launch_bounds__(256) k_curve(uint32_t n, const uint32_t *__restrict__ in, uint32_t wi, uint32_t *__restrict__ out, uint32_t wo) {
    using E = Ec29<C>;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        const uint32_t *c = in + (size_t)i * wi;
        uint32_t *o = out + (size_t)i * wo;
        if constexpr (OP == OP_CHAIN || OP == OP_CHAINS) {
            uint32_t cnt = c[0];
            const uint32_t room = (wi - 1u) / CALC_ENTRY_WORDS;
            if (cnt > room) cnt = room;
            xyzz29_t acc = E::identity();
#pragma unroll 1
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t *w = c + 1 + (size_t)j * CALC_ENTRY_WORDS;
                const affine_t q = calc_entry(w);
                acc = OP == OP_CHAIN ? E::madd(acc, E::load(q, w[16] != 0)) : E::madd_signed(acc, E::load_raw(q), w[16] != 0);
            }
            st32(o, E::pack(acc));
        } else if constexpr (OP == OP_CHAINF || OP == OP_CHAINF_RAW) {
            uint32_t cnt = c[33];
            const uint32_t room = (wi - 34u) / CALC_ENTRY_WORDS;
            if (cnt > room) cnt = room;
            const xyzz_t init = ld32(c + 1);
            bool exc = false;
            xyzz29_t acc = E::identity();
            if (cnt) acc = calc_chainf<C>(c[0] ? &init : nullptr, cnt, c + 34, exc);
            if constexpr (OP == OP_CHAINF) {
                st32(o, E::pack(acc));
                o[32] = exc ? 1u : 0u;
            } else {
                st9(o, acc.x);
                st9(o + 9, acc.y);
                st9(o + 18, acc.zz);
                st9(o + 27, acc.zzz);
                o[36] = exc ? 1u : 0u;
            }
        } else if constexpr (OP == OP_ADDP) {
            st32(o, E::pack(E::add(E::unpack(ld32(c)), E::unpack(ld32(c + 32)))));
        } else if constexpr (OP == OP_DBLP) {
            st32(o, E::pack(E::dbl(E::unpack(ld32(c)))));
        } else if constexpr (OP == OP_TFORM) {
            const affine_t t = E::table_form(calc_entry(c));
            st8(o, t.x);
            st8(o + 8, t.y);
        } else if constexpr (OP == OP_XYZZ) {
            st32(o, E::to_xyzz(E::unpack(ld32(c))));
        }
    }
}

struct OpInfo {
    const char *name;
    int op;
    bool curve;
    uint32_t wi, wo;        // words per case in / out; for the chains `wi` is the smallest admissible (header + one entry)
    bool variable;          // chains: any in_words >= wi
};
const OpInfo OPS[] = {
    {"mul", OP_MUL, false, 18, 9, false},       {"mul_ni", OP_MUL_NI, false, 18, 9, false}, {"sqr", OP_SQR, false, 9, 9, false},
    {"sqr_ni", OP_SQR_NI, false, 9, 9, false},  {"mul2", OP_MUL2, false, 36, 9, false},     {"norm", OP_NORM, false, 9, 9, false},
    {"add", OP_ADD, false, 18, 9, false},       {"canon", OP_CANON, false, 9, 8, false},    {"redlazy", OP_REDLAZY, false, 9, 9, false},
    {"unpack", OP_UNPACK, false, 8, 9, false},  {"pack", OP_PACK, false, 9, 8, false},      {"mul8", OP_MUL8, false, 16, 8, false},
    {"mul8_ni", OP_MUL8_NI, false, 16, 8, false}, {"sub", OP_SUB, false, 18, 9, false},     {"neg", OP_NEG, false, 9, 9, false},
    {"chain", OP_CHAIN, true, 1 + 17, 32, true}, {"chains", OP_CHAINS, true, 1 + 17, 32, true},
    {"chainf", OP_CHAINF, true, 34 + 17, 33, true}, {"chainf_raw", OP_CHAINF_RAW, true, 34 + 17, 37, true},
    {"addp", OP_ADDP, true, 64, 32, false},     {"dblp", OP_DBLP, true, 32, 32, false},     {"tform", OP_TFORM, true, 16, 16, false},
    {"xyzz", OP_XYZZ, true, 32, 32, false},
};

struct Launch {
    uint32_t n, wi, wo;
    const uint32_t *in;
    uint32_t *out;
    dim3 grid() const { return dim3((n + 255u) / 256u); }
};

template <class P, int OP>
void go_field(const Launch &l) { hipLaunchKernelGGL((k_field<P, OP>), l.grid(), dim3(256), 0, 0, l.n, l.in, l.wi, l.out, l.wo); }
template <class C, int OP>
void go_curve(const Launch &l) { hipLaunchKernelGGL((k_curve<C, OP>), l.grid(), dim3(256), 0, 0, l.n, l.in, l.wi, l.out, l.wo); }

template <class P>
bool launch_field(int op, uint32_t cp, uint32_t e, const Launch &l) {
    switch (op) {
        case OP_MUL: go_field<P, OP_MUL>(l); return true;
        case OP_MUL_NI: go_field<P, OP_MUL_NI>(l); return true;
        case OP_SQR: go_field<P, OP_SQR>(l); return true;
        case OP_SQR_NI: go_field<P, OP_SQR_NI>(l); return true;
        case OP_MUL2: go_field<P, OP_MUL2>(l); return true;
        case OP_NORM: go_field<P, OP_NORM>(l); return true;
        case OP_ADD: go_field<P, OP_ADD>(l); return true;
        case OP_CANON: go_field<P, OP_CANON>(l); return true;
        case OP_REDLAZY: go_field<P, OP_REDLAZY>(l); return true;
        case OP_UNPACK: go_field<P, OP_UNPACK>(l); return true;
        case OP_PACK: go_field<P, OP_PACK>(l); return true;
        case OP_MUL8: go_field<P, OP_MUL8>(l); return true;
        case OP_MUL8_NI: go_field<P, OP_MUL8_NI>(l); return true;
        default: break;
    }
    const bool neg = op == OP_NEG;
#define DEVCALC_TRY(CP, E)                                                                                                       \
    if (cp == CP && e == E) {                                                                                                    \
        if (neg) hipLaunchKernelGGL((k_sub<P, CP, E, true>), l.grid(), dim3(256), 0, 0, l.n, l.in, l.wi, l.out, l.wo);           \
        else hipLaunchKernelGGL((k_sub<P, CP, E, false>), l.grid(), dim3(256), 0, 0, l.n, l.in, l.wi, l.out, l.wo);              \
        return true;                                                                                                             \
    }
    SRS_CALC_SUB_PAIRS(DEVCALC_TRY)
#undef DEVCALC_TRY
    return false;
}

template <class C>
bool launch_curve(int op, const Launch &l) {
    switch (op) {
        case OP_CHAIN: go_curve<C, OP_CHAIN>(l); return true;
        case OP_CHAINS: go_curve<C, OP_CHAINS>(l); return true;
        case OP_CHAINF: go_curve<C, OP_CHAINF>(l); return true;
        case OP_CHAINF_RAW: go_curve<C, OP_CHAINF_RAW>(l); return true;
        case OP_ADDP: go_curve<C, OP_ADDP>(l); return true;
        case OP_DBLP: go_curve<C, OP_DBLP>(l); return true;
        case OP_TFORM: go_curve<C, OP_TFORM>(l); return true;
        case OP_XYZZ: go_curve<C, OP_XYZZ>(l); return true;
        default: return false;
    }
}

}  // namespace

// bit 0: the chained bodies of Fp29 are compiled in; bit 1: the FIPS body of Fp::mul is (it is whenever the device pass compiles field.cuh)
extern "C" int devcalc_info() {
    return 1 | 2;           // without SRS_F29_CHAIN this file does not compile (see the #error above)
}

// Runs `n` cases of one operation in one launch on the null stream.  Returns 0, a hipError_t, or -1: unknown operation / field / (cp, e),
// -2: words per case do not fit the operation.  which: "Fr" / "Fq" for the field operations, "Bn256" / "Grumpkin" for the curve ones.
extern "C" int devcalc_run(const char *op, const char *which, unsigned cp, unsigned e, unsigned n, const uint32_t *in, unsigned in_words,
                           uint32_t *out, unsigned out_words) {
    const OpInfo *info = nullptr;
    for (const OpInfo &o : OPS)
        if (strcmp(o.name, op) == 0) info = &o;
    if (!info) return -1;
    if (out_words != info->wo || (info->variable ? in_words < info->wi : in_words != info->wi)) return -2;
    const int w = strcmp(which, info->curve ? "Bn256" : "Fr") == 0 ? 0 : strcmp(which, info->curve ? "Grumpkin" : "Fq") == 0 ? 1 : -1;
    if (w < 0) return -1;
    if (n == 0) return 0;
    const size_t bi = (size_t)n * in_words * sizeof(uint32_t), bo = (size_t)n * out_words * sizeof(uint32_t);
    uint32_t *din = nullptr, *dout = nullptr;
    hipError_t rc = hipMalloc((void **)&din, bi);
    if (rc == hipSuccess) rc = hipMalloc((void **)&dout, bo);
    if (rc == hipSuccess) rc = hipMemcpy(din, in, bi, hipMemcpyHostToDevice);
    if (rc == hipSuccess) rc = hipMemset(dout, 0, bo);
    bool known = true;
    if (rc == hipSuccess) {
        const Launch l{n, in_words, out_words, din, dout};
        if (info->curve) known = w == 0 ? launch_curve<Bn256>(info->op, l) : launch_curve<Grumpkin>(info->op, l);
        else known = w == 0 ? launch_field<FrP>(info->op, cp, e, l) : launch_field<FqP>(info->op, cp, e, l);
        if (known) {
            rc = hipGetLastError();
            if (rc == hipSuccess) rc = hipDeviceSynchronize();
            if (rc == hipSuccess) rc = hipMemcpy(out, dout, bo, hipMemcpyDeviceToHost);
        }
    }
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
    if (!known) return -1;
    return (int)rc;
}
