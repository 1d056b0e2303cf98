// field29_audit.h -- TEST INFRASTRUCTURE: the bound audit of the 9 x 29-bit field form (csrc/field29.cuh), compiled only into the
// emulator's audit build (-DSRS_EMU -DSRS_F29_AUDIT, tests/emu/Makefile: libsirius_emu_audit.so).
//
// Every f29_t carries a SHADOW next to its limbs: the upper bound its producer DECLARES for the value (in units of P, exclusive)
// and for the limbs (the largest of limbs 0..7, and limb 8).  Every operation of Fp29 derives the shadow of its result from its
// operands' shadows exactly as its comment in field29.cuh states, and checks its stated precondition on the operands' shadows --
// on the declared bounds, never on the data: uniform inputs keep a lazy sum near half its bound, and a product of canonical
// operands comes out near 1.0 P, so values cannot show an error in the bound bookkeeping of a caller (emit_sweep_source); the
// bounds can, and one run of a straight-line program visits every operation.
//
// A violation does not abort: it is counted per kind, and the first site of each kind (file:line of the call, i.e. the line of the
// emitted program) is kept.  srs_emu_f29_audit (jit_emu.cpp) resets and reads the table; a run-time compiled unit has a table of
// its own (it is a separate shared object) which the emulator's launcher drains into the library's after every launch.
#pragma once
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <unordered_map>

namespace srs {
namespace f29_audit {

enum Kind : int {
    MUL_VALUE = 0,     // mul / sqr / mul2: A * B (+ C * D) >= 2^261 / P (in units of P^2)
    MUL_LIMBS,         // mul: not (a_i < 2^31, b_j < 2^29 or both < 2^30); sqr: a_i >= 2^30; mul2: a_i, c_i >= 2^30 or b_j, d_j >= 2^29
    ADD_WRAP,          // add_lazy / sub_lazy / neg_lazy: a 32-bit limb of the result can wrap
    SUB_BOUND,         // sub_lazy / neg_lazy <CP, E>: the subtrahend's bound exceeds CP
    SUB_LIMBS,         // sub_lazy / neg_lazy <CP, E>: b_i >= 2^(29+E) (i < 8) or b_8 > top limb of CP p - 2^E
    NORMALIZE,         // normalize: an input limb >= 2^32 - 8, or the value does not fit nine limbs (top limb >= 2^32)
    REDUCE_RANGE,      // reduce_lazy: limbs >= 2^29 or top limb >= 2^31
    CANONICAL_RANGE,   // to_canonical_fe: not a normalised value < 4P
    PACK_RANGE,        // pack: not a normalised value < 2^256
    UNTRACKED,         // an operand without a shadow (limbs written directly, or an LDS word nobody stored): taken as normalised, < 2P
    CHECKED,           // not a violation: the number of products whose precondition was checked (a run that counts none audited nothing)
    KIND_COUNT
};
constexpr int SITE_BYTES = 160;

struct Shadow {
    double bound = -1.0;        // value < bound * P; < 0: untracked
    uint64_t lo = 0, top = 0;   // limbs 0..7 <= lo, limb 8 <= top (64-bit so that a wrap of the 32-bit limb shows)
};

struct Table {
    std::atomic<uint64_t> count[KIND_COUNT];
    std::mutex m;
    char site[KIND_COUNT][SITE_BYTES];
    Table() { clear(); }
    void clear() {
        std::lock_guard<std::mutex> g(m);
        for (int k = 0; k < KIND_COUNT; ++k) { count[k] = 0; site[k][0] = 0; }
    }
    void add(int kind, uint64_t n, const char *where) {
        if (count[kind].fetch_add(n) == 0) {
            std::lock_guard<std::mutex> g(m);
            if (!site[kind][0]) std::snprintf(site[kind], SITE_BYTES, "%.159s", where);
        }
    }
};
inline Table &table() {
    static Table t;
    return t;
}
inline void report(int kind, const char *op, const char *file, int line, double x, double y) {
    char buf[SITE_BYTES];
    const char *base = std::strrchr(file, '/');
    std::snprintf(buf, sizeof buf, "%s:%d %s (%.6g, %.6g)", base ? base + 1 : file, line, op, x, y);
    table().add(kind, 1, buf);
}
// read (and optionally reset) a table: counts[KIND_COUNT], sites[KIND_COUNT][SITE_BYTES]
inline void read_table(int reset, uint64_t *counts, char *sites) {
    Table &t = table();
    {
        std::lock_guard<std::mutex> g(t.m);
        for (int k = 0; k < KIND_COUNT; ++k) {
            if (counts) counts[k] = t.count[k];
            if (sites) std::memcpy(sites + (size_t)k * SITE_BYTES, t.site[k], SITE_BYTES);
        }
    }
    if (reset) t.clear();
}

// the shadows of the sweep accumulators' LDS words (sw_store / sw_load, rowprog_dev.cuh), keyed by the address of limb 0.  The
// emulator runs a block's threads as fibers of one OS thread and `__shared__` is thread_local, so the table is thread_local too.
inline std::unordered_map<const void *, Shadow> &lds_shadows() {
    static thread_local std::unordered_map<const void *, Shadow> m;
    return m;
}

template <class P>
struct Field {
    static long double modulus() {                           // P as a long double (64-bit mantissa: relative error 2^-64)
        long double v = 0;
        for (int j = 7; j >= 0; --j) v = v * 4294967296.0L + (long double)P::p(j);
        return v;
    }
    // 2^261 / P, the exact ratio of THIS field (field29.cuh says "> 165"): what A * B must stay below
    static double ratio() {
        static const double r = (double)(__builtin_ldexpl(1.0L, 261) / modulus());
        return r;
    }
    // the top limb (value >> 232) of a value < bound * P
    static uint64_t top_of(double bound) {
        static const long double ptop = __builtin_ldexpl(modulus(), -232);
        return bound <= 0 ? 0 : (uint64_t)((long double)bound * ptop);
    }
    static Shadow normalised(double bound) { return Shadow{bound, (1u << 29) - 1u, top_of(bound)}; }
};

// The shadow arithmetic of Fp29<P>'s operations (G = Fp29<P>; T = f29_t).  Called through SRS_F29_CHECK at the end of each.
template <template <class> class G29, class P>
struct Ops {
    using G = G29<P>;
    using Fd = Field<P>;
    static constexpr uint64_t LIMB = 1ull << 29, WORD = 1ull << 32;

    template <class T>
    static Shadow get(const T &a, const char *op, const char *file, int line) {
        if (a.sh.bound >= 0) return a.sh;
        report(UNTRACKED, op, file, line, 0, 0);
        return Fd::normalised(2.0);
    }
    static uint64_t mx(const Shadow &s) { return s.lo > s.top ? s.lo : s.top; }

    template <class T> static void zero(T &o) { o.sh = Shadow{0.0, 0, 0}; }
    template <class T> static void unpack(T &o) { o.sh = Fd::normalised(1.0); }           // a loaded element: canonical
    template <class T> static void select(T &o, const T &x, const T &y) {
        const Shadow a = get(x, "select", "-", 0), b = get(y, "select", "-", 0);
        o.sh = Shadow{a.bound > b.bound ? a.bound : b.bound, a.lo > b.lo ? a.lo : b.lo, a.top > b.top ? a.top : b.top};
    }
    // mul: A * B < 2^261 * P, i.e. (A / P) (B / P) < 2^261 / P;  limbs a_i < 2^31, b_j < 2^29 (the column sums are symmetric in
    // the operands, so either way round) or both < 2^30.  -> < 2P, normalised
    template <class T> static void mul(T &o, const T &a, const T &b, const char *file, int line) {
        const Shadow x = get(a, "mul", file, line), y = get(b, "mul", file, line);
        ++table().count[CHECKED];
        if (!(x.bound * y.bound < Fd::ratio())) report(MUL_VALUE, "mul", file, line, x.bound, y.bound);
        const uint64_t ma = mx(x), mb = mx(y);
        if (!((ma < 4 * LIMB && mb < LIMB) || (mb < 4 * LIMB && ma < LIMB) || (ma < 2 * LIMB && mb < 2 * LIMB)))
            report(MUL_LIMBS, "mul", file, line, (double)ma, (double)mb);
        o.sh = Fd::normalised(2.0);
    }
    template <class T> static void sqr(T &o, const T &a, const char *file, int line) {
        const Shadow x = get(a, "sqr", file, line);
        ++table().count[CHECKED];
        if (!(x.bound * x.bound < Fd::ratio())) report(MUL_VALUE, "sqr", file, line, x.bound, x.bound);
        if (!(mx(x) < 2 * LIMB)) report(MUL_LIMBS, "sqr", file, line, (double)mx(x), 0);
        o.sh = Fd::normalised(2.0);
    }
    // mul2: A * B + C * D < 2^261 * P;  a_i, c_i < 2^30,  b_j, d_j < 2^29
    template <class T> static void mul2(T &o, const T &a, const T &b, const T &c, const T &d, const char *file, int line) {
        const Shadow x = get(a, "mul2", file, line), y = get(b, "mul2", file, line), z = get(c, "mul2", file, line), w = get(d, "mul2", file, line);
        ++table().count[CHECKED];
        if (!(x.bound * y.bound + z.bound * w.bound < Fd::ratio())) report(MUL_VALUE, "mul2", file, line, x.bound * y.bound, z.bound * w.bound);
        if (!(mx(x) < 2 * LIMB && mx(z) < 2 * LIMB && mx(y) < LIMB && mx(w) < LIMB))
            report(MUL_LIMBS, "mul2", file, line, (double)(mx(x) > mx(z) ? mx(x) : mx(z)), (double)(mx(y) > mx(w) ? mx(y) : mx(w)));
        o.sh = Fd::normalised(2.0);
    }
    template <class T> static void add_lazy(T &o, const T &a, const T &b, const char *file, int line) {
        const Shadow x = get(a, "add_lazy", file, line), y = get(b, "add_lazy", file, line);
        o.sh = Shadow{x.bound + y.bound, x.lo + y.lo, x.top + y.top};
        if (o.sh.lo >= WORD || o.sh.top >= WORD) report(ADD_WRAP, "add_lazy", file, line, (double)o.sh.lo, (double)o.sh.top);
    }
    // sub_lazy<CP, E> (a == nullptr: neg_lazy): a - b + CP p needs b <= CP p, b_i < 2^(29+E) (i < 8), b_8 <= top limb of CP p - 2^E;
    // -> a + CP, limbs <= a_i + the limbs of the raised constant
    template <uint32_t CP, uint32_t E, class T> static void sub_lazy(T &o, const T *a, const T &b, const char *file, int line) {
        const char *op = a ? "sub_lazy" : "neg_lazy";
        const Shadow x = a ? get(*a, op, file, line) : Shadow{0.0, 0, 0}, y = get(b, op, file, line);
        if (y.bound > (double)CP) report(SUB_BOUND, op, file, line, y.bound, (double)CP);
        if (y.lo >= (LIMB << E) || y.top > (uint64_t)G::kpb(CP, E, 8)) report(SUB_LIMBS, op, file, line, (double)y.top, (double)G::kpb(CP, E, 8));
        uint64_t klo = 0;
        for (int i = 0; i < 8; ++i) klo = klo > G::kpb(CP, E, i) ? klo : G::kpb(CP, E, i);
        o.sh = Shadow{x.bound + (double)CP, x.lo + klo, x.top + G::kpb(CP, E, 8)};
        if (o.sh.lo >= WORD || o.sh.top >= WORD) report(ADD_WRAP, op, file, line, (double)o.sh.lo, (double)o.sh.top);
    }
    // normalize: limbs < 2^32 - 8 in (the carry of the limb below is < 8); the value must fit nine limbs
    template <class T> static void normalize(T &o, const T &a, const char *file, int line) {
        const Shadow x = get(a, "normalize", file, line);
        const uint64_t by_value = Fd::top_of(x.bound), by_limbs = x.top + 8;
        if (x.lo >= WORD - 8 || by_value >= WORD) report(NORMALIZE, "normalize", file, line, (double)x.lo, (double)by_value);
        o.sh = Shadow{x.bound, x.lo < LIMB ? x.lo : LIMB - 1, by_value < by_limbs ? by_value : by_limbs};
    }
    template <class T> static void reduce_lazy(T &o, const T &a, const char *file, int line) {
        const Shadow x = get(a, "reduce_lazy", file, line);
        if (x.lo >= LIMB || x.top >= 4 * LIMB) report(REDUCE_RANGE, "reduce_lazy", file, line, (double)x.lo, (double)x.top);
        o.sh = Fd::normalised(2.0);
    }
    template <class T> static void to_canonical(const T &a, const char *file, int line) {
        const Shadow x = get(a, "to_canonical_fe", file, line);
        if (x.bound > 4.0 || x.lo >= LIMB) report(CANONICAL_RANGE, "to_canonical_fe", file, line, x.bound, (double)x.lo);
    }
    template <class T> static void pack(const T &a, const char *file, int line) {
        const Shadow x = get(a, "pack", file, line);
        if (x.lo >= LIMB || x.top >= (1ull << 24)) report(PACK_RANGE, "pack", file, line, (double)x.lo, (double)x.top);
    }
};

}  // namespace f29_audit
}  // namespace srs
