// field29_check.cpp -- TEST INFRASTRUCTURE (host build of field29.cuh / curve29.cuh through the emulator headers).
// A line-oriented calculator: tests/test_field29_host.py feeds operands chosen at the stated bounds of the lazy 9 x 29-bit
// arithmetic and checks every result with Python integers.
//   mul F a[9] b[9] | sqr F a[9] | norm F a[9] | add F a[9] b[9] | sub F CP E a[9] b[9] | neg F CP E b[9] | canon F a[9]
//   unpack F w[8] | pack F a[9] | redlazy F a[9]
//   mul8 F a[8] b[8]             : Fp<P>::mul on the 8 x 32-bit form (here the host 4 x 64 CIOS; on the device the generated FIPS body)
//   mul2 F a[9] b[9] c[9] d[9]   : (a b + c d) / 2^261 with one reduction
//   chain C n (w[16] neg){n}     : identity + n mixed additions of table-form points, lazy in between -> packed XYZZ (32 words)
//   chains C n (w[16] neg){n}    : the same through madd_signed / load_raw (what k_accum0 runs)
//   chainf C has_init [init[32]] n (w[16] neg){n} : the chain as accumulate_part runs it (field29_calc.h: calc_chainf), n >= 1 -> packed + exc
//   chainf_raw ...               : the same, printing the unpacked 4 x 9 limbs (x y zz zzz) + exc: the bounds of the "garbage" after an exception
//   addp C a[32] b[32]           : Ec29::add of two packed partial sums -> packed
//   dblp C a[32]                 : Ec29::dbl -> packed
//   tform C w[16]                : table_form of an ABI affine point -> 16 words
//   xyzz C a[32]                 : packed R'-form -> ABI XYZZ (to_xyzz)
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hipemu.h"
#include "field29_calc.h"

using namespace srs;

template <class P>
static f29_t rd9(std::istringstream &in) {
    f29_t a;
    for (int i = 0; i < 9; ++i) { unsigned long long v; in >> std::hex >> v; a.v[i] = (uint32_t)v; }
    return a;
}
static fe_t rd8(std::istringstream &in) {
    fe_t a;
    for (int i = 0; i < 8; ++i) { unsigned long long v; in >> std::hex >> v; a.v[i] = (uint32_t)v; }
    return a;
}
static void pr(const uint32_t *v, int n) {
    for (int i = 0; i < n; ++i) std::printf("%x%c", v[i], i + 1 < n ? ' ' : '\n');
}

template <class P, uint32_t CP, uint32_t E>
static bool try_sub(uint32_t cp, uint32_t e, bool neg, const f29_t &a, const f29_t &b) {
    if (cp != CP || e != E) return false;
    f29_t o = neg ? Fp29<P>::template neg_lazy<CP, E>(b) : Fp29<P>::template sub_lazy<CP, E>(a, b);
    pr(o.v, 9);
    return true;
}

template <class P>
static void field_op(const std::string &op, std::istringstream &in) {
    using G = Fp29<P>;
    if (op == "mul") { f29_t a = rd9<P>(in), b = rd9<P>(in); pr(G::mul(a, b).v, 9); }
    else if (op == "mul2") { f29_t a = rd9<P>(in), b = rd9<P>(in), c = rd9<P>(in), d = rd9<P>(in); pr(G::mul2(a, b, c, d).v, 9); }
    else if (op == "sqr") { f29_t a = rd9<P>(in); pr(G::sqr(a).v, 9); }
    else if (op == "norm") { f29_t a = rd9<P>(in); pr(G::normalize(a).v, 9); }
    else if (op == "add") { f29_t a = rd9<P>(in), b = rd9<P>(in); pr(G::add_lazy(a, b).v, 9); }
    else if (op == "canon") { f29_t a = rd9<P>(in); pr(G::to_canonical_fe(a).v, 8); }
    else if (op == "redlazy") { f29_t a = rd9<P>(in); pr(G::reduce_lazy(a).v, 9); }
    else if (op == "unpack") { fe_t a = rd8(in); pr(G::unpack(a).v, 9); }
    else if (op == "pack") { f29_t a = rd9<P>(in); pr(G::pack(a).v, 8); }
    else if (op == "mul8") { fe_t a = rd8(in), b = rd8(in); pr(Fp<P>::mul(a, b).v, 8); }
    else if (op == "sub" || op == "neg") {
        unsigned cp, e;
        in >> std::dec >> cp >> e;
        const bool neg = op == "neg";
        f29_t a = neg ? G::zero() : rd9<P>(in), b = rd9<P>(in);
        bool ok = false;
#define SRS_CALC_TRY(CP, E) ok = ok || try_sub<P, CP, E>(cp, e, neg, a, b);
        SRS_CALC_SUB_PAIRS(SRS_CALC_TRY)
#undef SRS_CALC_TRY
        if (!ok) std::printf("unsupported\n");
    } else std::printf("unsupported\n");
}

template <class C>
static void curve_op(const std::string &op, std::istringstream &in) {
    using E = Ec29<C>;
    auto rdp = [&](xyzz_t &p) { p.x = rd8(in); p.y = rd8(in); p.zz = rd8(in); p.zzz = rd8(in); };
    auto prp = [&](const xyzz_t &p) { uint32_t w[32]; std::memcpy(w, &p, sizeof p); pr(w, 32); };
    if (op == "chain" || op == "chains") {
        unsigned n;
        in >> std::dec >> n;
        xyzz29_t acc = E::identity();
        for (unsigned i = 0; i < n; ++i) {
            affine_t q;
            q.x = rd8(in);
            q.y = rd8(in);
            unsigned neg;
            in >> std::dec >> neg;
            acc = op == "chain" ? E::madd(acc, E::load(q, neg != 0)) : E::madd_signed(acc, E::load_raw(q), neg != 0);
        }
        prp(E::pack(acc));
    } else if (op == "chainf" || op == "chainf_raw") {
        unsigned has_init, n;
        in >> std::dec >> has_init;
        xyzz_t init;
        if (has_init) rdp(init);
        in >> std::dec >> n;
        std::vector<uint32_t> ent((size_t)n * CALC_ENTRY_WORDS);
        for (unsigned i = 0; i < n; ++i) {
            for (int j = 0; j < 16; ++j) { unsigned long long v; in >> std::hex >> v; ent[i * CALC_ENTRY_WORDS + j] = (uint32_t)v; }
            unsigned neg;
            in >> std::dec >> neg;
            ent[i * CALC_ENTRY_WORDS + 16] = neg;
        }
        if (n == 0) { std::printf("unsupported\n"); return; }
        bool exc;
        const xyzz29_t acc = calc_chainf<C>(has_init ? &init : nullptr, n, ent.data(), exc);
        uint32_t w[37];
        if (op == "chainf") {
            const xyzz_t o = E::pack(acc);
            std::memcpy(w, &o, sizeof o);
            w[32] = exc;
            pr(w, 33);
        } else {
            std::memcpy(w, &acc, sizeof acc);
            w[36] = exc;
            pr(w, 37);
        }
    } else if (op == "addp") {
        xyzz_t a, b;
        rdp(a); rdp(b);
        prp(E::pack(E::add(E::unpack(a), E::unpack(b))));
    } else if (op == "dblp") {
        xyzz_t a;
        rdp(a);
        prp(E::pack(E::dbl(E::unpack(a))));
    } else if (op == "tform") {
        affine_t q;
        q.x = rd8(in);
        q.y = rd8(in);
        affine_t t = E::table_form(q);
        uint32_t w[16];
        std::memcpy(w, &t, sizeof t);
        pr(w, 16);
    } else if (op == "xyzz") {
        xyzz_t a;
        rdp(a);
        prp(E::to_xyzz(E::unpack(a)));
    } else std::printf("unsupported\n");
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, which;
        in >> op >> which;
        if (which == "Fr") field_op<FrP>(op, in);
        else if (which == "Fq") field_op<FqP>(op, in);
        else if (which == "Bn256") curve_op<Bn256>(op, in);
        else if (which == "Grumpkin") curve_op<Grumpkin>(op, in);
        else std::printf("unsupported\n");
        std::fflush(stdout);
    }
    return 0;
}
