// msm.hip -- Pedersen vector commitment  C = sum_i v[i] * ck[i]  on gfx950.
//
// Replaces the body of `CommitmentKey::commit` = `best_multiexp(v, &ck[..v.len()]).to_affine()`
// (reference src/commitment.rs:81-90; call sites src/plonk/mod.rs:441-447,
// src/nifs/sangria/mod.rs:151-154).  Group arithmetic is exact, so any evaluation order gives the
// reference's affine point bit for bit.
//
// MI355X-first design (not halo2's chunk-per-thread serial Pippenger):
//   * The commitment key is static across fold steps, and HBM is 288 GB: at key creation every
//     base is expanded into the 16 window multiples  T[w][i] = 2^(16 w) * P_i  (affine, 16x the
//     key size).  All 16 windows of a scalar then land in ONE shared set of 2^15 signed-digit
//     buckets: no per-window bucket sets, no Horner doublings, one bucket reduction per MSM.
//   * scalars -> 16 signed 16-bit digits (k_digits); zero digits are skipped like halo2 does.
//   * counting sort of the (bucket, table-index) pairs with a 128 KiB LDS histogram per
//     workgroup (k_hist / k_scatter): hot buckets (0/1/small witnesses) are
//     aggregated in LDS and cost one global atomic per tile, not one per entry.
//   * load-balanced bucket accumulation (k_accum0): one thread per (bucket, part) with at most
//     L0 gathered mixed adds, so a bucket holding 20 % of all entries is spread over thousands
//     of threads; partial sums are combined by further levels (k_accum1) and a wavefront-level
//     strided sum + 64-lane shuffle tree (k_accum_final).
//   * bucket reduction  sum_b (b+1) B_b  via the 2-D row/column split (k_rowcol) and log-depth
//     suffix scans in LDS (k_reduce_final); the XYZZ result is normalised on the host.
//   * everything after k_accum0 is a chain of ~30 DEPENDENT additions on a nearly idle chip: those kernels give every
//     addition to a QUAD of lanes (Ec::add_quad, curve.cuh: 4 levels of independent products exchanged with DPP
//     quad_perm moves), 3.9 us instead of 9.8 us per addition.
// Batched entry: the d-1 cross-term commitments share one base prefix and run
// as one set of launches (grid.y / grid.z = batch index).
// r04: the sets of a STREAMED commit (the witness comes up from host memory in chunks, capi.hip: commit_streamed) run in SLOT MODE:
// every bucket owns 2^6 persistent partial sums in HBM, a level-0 part adds its entries into "its" slot (k_accum0s), so the accumulation
// levels / wave pass / bucket fold that every chunk used to run are ONE reduction of the slots per commit (k_slot_reduce); the plan of a
// set (k_plan_s) picks the part length on the device; parts beyond the slots (hot buckets) go through the level kernels into the
// bucket's last slot, launched only when the key expects them (msm.h: overflow_missed / note_commit).  Whole MSMs of >= 2^23 scalars
// take the 13 x 20-bit "wide" windows over a second table (16 virtual MSMs of 2^15 buckets each).
// Compact keys (tuning msm_compact = 1 at creation, msm.h): 8 stored windows; k_digits splits the scalar with the curve endomorphism
// (glv.cuh), rows 8..15 gather phi of windows 0..7 -- the payload carries a flag, level 0 multiplies the gathered x by beta (k_accum0c /
// k_accum0sc).  Everything between the digits and level 0, and everything after it, is shared with full keys.  msm_compact = 2: such a
// key may also hold a wide table of 7 windows; the segment passes then split the scalar themselves (k_seg_pass<., ., true>: 14 rows).
// Host driver (end of this file): enqueue() picks one of three flows (enqueue_t: levels, enqueue_slots_t: slot mode, enqueue_wide_t).  Each
// computes its shape once (*_shape: sizes, grids and every tunable), carves the key's arena by its one buffer list (*_layout, also the
// sizer behind reserve()) and runs the shared stages: sort_front, accum_levels, reduce_buckets, land.
// The 29-bit products of THIS translation unit chain every column's multiply-accumulates from the previous column's carry (inline
// v_mad_u64_u32, field29.cuh): no 64-bit join per column, 127 instead of 132 VGPRs in k_accum0 / k_accum0s (4 waves per SIMD instead of
// 3): 13.85 -> 14.4 G mixed additions/s, profiles/r04_ab_slots_cuts.txt; one asm statement per RUN of multiply-accumulates, not per
// instruction (hipcc pads each statement with an s_nop, ~1 cycle each): + 2.7 % more, profiles/r04_ab_chain_blocks.txt.  Device code only;
// host and emulator builds keep the C form.
#define SRS_F29_CHAIN 1
#include "msm.h"
#include "tuning.h"
#include "curve29.cuh"
#include "prof.h"

#include <algorithm>
#include <cstdlib>
#include <numeric>
#include <vector>

namespace srs {
namespace msm {

// ---------------------------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t upper_bucket(const uint32_t *__restrict__ tp, uint32_t t) {
    // largest b in [0, NBUCKET) with tp[b] <= t   (tp is non-decreasing, tp[0] = 0, t < tp[NBUCKET])
    uint32_t lo = 0, hi = NBUCKET;
    while (hi - lo > 1) {
        uint32_t mid = (lo + hi) >> 1;
        if (tp[mid] <= t) lo = mid; else hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------
// key expansion: T[w][i] = 2^(16 w) P_i
// ---------------------------------------------------------------------------------------------
template <class C>
__global__ void k_table_step(const affine_t *__restrict__ prev, xyzz_t *__restrict__ tmp, uint32_t n, int nbits) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    affine_t p = prev[i];
    xyzz_t a;
    if (Ec<C>::is_identity(p)) {
        a = Ec<C>::identity();
    } else {
        a = Ec<C>::dbl_affine(p);
        for (int k = 1; k < nbits; ++k) a = Ec<C>::dbl(a);
    }
    tmp[i] = a;
}

// batch normalisation XYZZ -> affine, NORM_G points per thread share one inversion
template <class C>
__global__ void k_normalize(const xyzz_t *__restrict__ in, affine_t *__restrict__ out, uint32_t n) {
    using F = typename C::F;
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    size_t lo = (size_t)g * NORM_G;
    if (lo >= n) return;
    uint32_t cnt = (uint32_t)((n - lo < NORM_G) ? (n - lo) : NORM_G);
    fe_t pre[NORM_G];
    fe_t acc = F::one();
    for (uint32_t j = 0; j < cnt; ++j) {
        pre[j] = acc;
        xyzz_t p = in[lo + j];
        if (!Ec<C>::is_identity(p)) acc = F::mul(acc, F::mul(p.zz, p.zzz));
    }
    fe_t inv = F::inv(acc);
    for (uint32_t j = cnt; j-- > 0;) {
        xyzz_t p = in[lo + j];
        affine_t o;
        if (Ec<C>::is_identity(p)) {
            o = Ec<C>::affine_identity();
        } else {
            fe_t i = F::mul(inv, pre[j]);                 // 1 / (zz * zzz)
            inv = F::mul(inv, F::mul(p.zz, p.zzz));
            o.x = F::mul(p.x, F::mul(i, p.zzz));
            o.y = F::mul(p.y, F::mul(i, p.zz));
        }
        out[lo + j] = o;
    }
}

// The finished table is kept in the R' = 2^261 Montgomery form of the 9 x 29-bit multiplier that k_accum0 runs on
// (field29.cuh): one pass over all NWIN * len entries when the key is created.  k_table_unform is the inverse, used by
// the few readers of the plain bases (srs_ck_get_bases / save_file, the on-curve count).
template <class C>
__global__ void k_table_form(affine_t *__restrict__ t, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    t[i] = Ec29<C>::table_form(t[i]);
}
template <class C>
__device__ __forceinline__ affine_t table_unform(const affine_t &q) {
    using G = typename C::F;
    fe_t c = G::one();
    for (int d = 0; d < 5; ++d) c = G::halve(c);          // 2^256 / 32 = 2^251 mod p as an integer: x 2^261 * 2^251 / 2^256 = x 2^256
    affine_t o;
    o.x = G::mul(q.x, c);
    o.y = G::mul(q.y, c);
    return o;
}
template <class C>
__global__ void k_table_unform(const affine_t *__restrict__ t, affine_t *__restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = table_unform<C>(t[i]);
}

// synthetic key: P_i = [h(seed, g)] G with g the GLOBAL index of local base i  (NOT the reference's
// SHAKE256 + hash_to_curve key, src/commitment.rs:55-79 -- hash_to_curve is [3P]; any valid points
// with no known small relation serve parity and timing)
__device__ __forceinline__ uint64_t splitmix64(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
template <class C>
__global__ void k_gen_bases(xyzz_t *__restrict__ tmp, uint32_t n, uint64_t seed, uint32_t rank, uint32_t world) {
    using F = typename C::F;
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint64_t g = Stripes{rank, world}.global_index((size_t)i);
    uint64_t st = seed ^ (g * 0x100000001b3ull + 0xcbf29ce484222325ull);
    uint32_t k[8];
    for (int j = 0; j < 4; ++j) {
        uint64_t v = splitmix64(st);
        k[2 * j] = (uint32_t)v;
        k[2 * j + 1] = (uint32_t)(v >> 32);
    }
    k[7] &= 0x0FFFFFFFu;   // < 2^252 < group order
    k[0] |= 1u;
    affine_t gen;
    gen.x = F::one();
    if (C::ID == 0) {
        gen.y = F::dbl(F::one());                                  // bn256 G1 generator (1, 2)
    } else {
        // grumpkin generator (1, sqrt(-16)) = 17631683881184975370165255887551781615748388533673675138860
        fe_t y;
        const uint32_t yc[8] = {0x823f272cu, 0x833fc48du, 0xf1181294u, 0x2d270d45u, 0x06a45d63u, 0xcf135e75u, 0x00000002u, 0u};
        for (int j = 0; j < 8; ++j) y.v[j] = yc[j];
        gen.y = F::to_mont(y);
    }
    tmp[i] = Ec<C>::mul_canon(k, gen);
}

// is_on_curve over a key (reference: load_or_setup_cache validates every point, src/commitment.rs:148-160)
template <class C>
__global__ void k_on_curve(const affine_t *__restrict__ pts, uint32_t n, uint32_t *__restrict__ bad) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!Ec<C>::is_on_curve(table_unform<C>(pts[i]))) atomicAdd(bad, 1u);
}

// ---------------------------------------------------------------------------------------------
// 1. scalars -> signed 16-bit digits
// dig[w * n + i] = 0xFFFF (zero digit) | (|d|-1) | sign << 15
// ---------------------------------------------------------------------------------------------
// the batch descriptor travels as a kernel argument (no host-to-device copies of pointer / length arrays per call)
struct BatchDesc {
    const fe_t *ptr[BATCH_ARGS];
    uint32_t n[BATCH_ARGS];
    uint32_t base[BATCH_ARGS];      // first base of MSM m inside the key (0 for the usual prefix commit; chunked commits slide it)
};

// compact keys: the NW signed WB-bit digits of one half (|k| < 2^127, sign `neg`) of the split scalar; put(w, mag, minus) takes digit w
// as its magnitude (0: a zero digit) and sign.  The half's sign goes into every digit, and the tie v = 2^(WB - 1) is broken by it: the
// code formats hold digits -(2^(WB - 1) - 1) .. 2^(WB - 1), so a negative half recodes |k| into -2^(WB - 1) .. 2^(WB - 1) - 1 before
// negating.  The top digit never carries out: tools/gen_glv_consts.py proves |k| < 2^126, so the top window of 8 x 16 bits holds at most
// 14 bits and that of 7 x 20 bits at most 6, plus the carry.
template <int WB, int NW, class Put>
__device__ __forceinline__ void recode_half(const uint32_t (&k)[4], bool neg, Put put) {
    static_assert(WB * NW >= 127 && WB <= 31, "the windows cover a half of the split scalar");
    constexpr uint32_t HALF = 1u << (WB - 1);
    const uint32_t top = neg ? HALF - 1u : HALF;      // largest v that stays a non-negative digit of |k|
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const int bit = WB * w, limb = bit >> 5, sh = bit & 31;
        uint32_t raw = k[limb] >> sh;
        if (sh + WB > 32 && limb + 1 < 4) raw |= k[limb + 1] << (32 - sh);
        const uint32_t v = (raw & (2u * HALF - 1u)) + carry;
        const bool borrow = v > top;
        const uint32_t mag = borrow ? 2u * HALF - v : v;
        const bool minus = borrow != neg;              // sign of the digit of the SIGNED half
        carry = borrow ? 1u : 0u;
        put(w, mag, minus);
    }
}
// ... as rows d[0], d[n], ..., d[7 n] of the 16-bit code format
__device__ __forceinline__ void recode_half16(const uint32_t (&k)[4], bool neg, uint16_t *__restrict__ d, size_t n) {
    recode_half<WBITS, NWIN_COMPACT>(k, neg, [&](int w, uint32_t mag, bool minus) {
        d[(size_t)w * n] = (uint16_t)(mag ? ((mag - 1u) | (minus ? 0x8000u : 0u)) : 0xFFFFu);
    });
}

template <class C, bool COMPACT>
__global__ void k_digits(BatchDesc bd, uint16_t *__restrict__ dig, size_t dig_stride, int is_mont, uint32_t rank, uint32_t world,
                         uint32_t *__restrict__ count_zero, uint32_t n_zero) {
    using S = typename C::S;
    uint32_t m = blockIdx.y;
    uint32_t n = bd.n[m];
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    // the bucket counters k_hist adds into start at zero: cleared here (k_digits precedes k_hist on the stream) instead of by a
    // memset launch of its own per MSM
    for (uint32_t j = (blockIdx.y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; j < n_zero; j += gridDim.x * gridDim.y * blockDim.x)
        count_zero[j] = 0;
    if (i >= n) return;
    fe_t s = bd.ptr[m][Stripes{rank, world}.global_index((size_t)i)];
    if (is_mont) s = S::from_mont(s);
    uint16_t *d = dig + (size_t)m * dig_stride;
    if (COMPACT) {                            // k = k1 + lambda k2: rows 0..7 from |k1|, rows 8..15 from |k2| (entries of phi(P), see k_scatter)
        const glv_t g = glv_decompose<C>(s);
        recode_half16(g.k1, g.neg1, d + i, n);
        recode_half16(g.k2, g.neg2, d + (size_t)NWIN_COMPACT * n + i, n);
        return;
    }
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < NWIN; ++w) {
        uint32_t raw = (s.v[w >> 1] >> ((w & 1) * 16)) & 0xFFFFu;
        uint32_t v = raw + carry;
        uint32_t code;
        if (v > 0x8000u) {
            code = ((0x10000u - v) - 1u) | 0x8000u;   // negative digit, magnitude 1..0x7FFF
            carry = 1;
        } else {
            code = v ? (v - 1u) : 0xFFFFu;            // positive digit 1..0x8000, or zero
            carry = 0;
        }
        d[(size_t)w * n + i] = (uint16_t)code;
    }
}

// ---------------------------------------------------------------------------------------------
// 2. counting sort by bucket, LDS histogram per workgroup
// grid = (tiles, NWIN, batch), block = SORT_THREADS
// ---------------------------------------------------------------------------------------------
// fn(i, code) for every digit slot i in [lo, hi): 8 digits per 16-byte load once the pointer is aligned (a 2-byte load per
// lane uses 1/8 of the load width: the digit streams are read by k_hist, k_scatter and k_group)
template <class Fn>
__device__ __forceinline__ void for_each_digit(const uint16_t *__restrict__ d, uint32_t lo, uint32_t hi, Fn fn) {
    uint32_t head = lo;
    while (head < hi && (reinterpret_cast<uintptr_t>(d + head) & 15u)) ++head;      // at most 7 unaligned slots
    for (uint32_t i = lo + threadIdx.x; i < head; i += blockDim.x) fn(i, (uint32_t)d[i]);
    const uint32_t nvec = (hi - head) / 8;
    const uint4 *v = reinterpret_cast<const uint4 *>(d + head);
    auto eight = [&](uint32_t q, const uint4 &x) {
        const uint32_t i0 = head + q * 8;
        fn(i0 + 0, x.x & 0xFFFFu); fn(i0 + 1, x.x >> 16);
        fn(i0 + 2, x.y & 0xFFFFu); fn(i0 + 3, x.y >> 16);
        fn(i0 + 4, x.z & 0xFFFFu); fn(i0 + 5, x.z >> 16);
        fn(i0 + 6, x.w & 0xFFFFu); fn(i0 + 7, x.w >> 16);
    };
    // four 16-byte loads in flight per thread (r04: one load per loop round left a workgroup with 16 loads in flight -- the digit streams
    // of a large chunk took 25 memory latencies per thread)
    uint32_t q = threadIdx.x;
    for (; q + 3 * blockDim.x < nvec; q += 4 * blockDim.x) {
        const uint4 x0 = v[q], x1 = v[q + blockDim.x], x2 = v[q + 2 * blockDim.x], x3 = v[q + 3 * blockDim.x];
        eight(q, x0); eight(q + blockDim.x, x1); eight(q + 2 * blockDim.x, x2); eight(q + 3 * blockDim.x, x3);
    }
    for (; q < nvec; q += blockDim.x) eight(q, v[q]);
    for (uint32_t i = head + nvec * 8 + threadIdx.x; i < hi; i += blockDim.x) fn(i, (uint32_t)d[i]);
}

__device__ __forceinline__ void tile_histogram(uint32_t *h, const uint16_t *__restrict__ d, uint32_t lo, uint32_t hi) {
    for (uint32_t b = threadIdx.x; b < NBUCKET; b += blockDim.x) h[b] = 0;
    __syncthreads();
    for_each_digit(d, lo, hi, [&](uint32_t, uint32_t code) {
        if (code != 0xFFFFu) atomicAdd(&h[code & 0x7FFFu], 1u);
    });
    __syncthreads();
}

__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 1)
    k_hist(const uint16_t *__restrict__ dig, size_t dig_stride, BatchDesc bd,
           uint32_t *__restrict__ count /* [batch][NBUCKET] */, uint32_t SORT_TILE,
           uint32_t *__restrict__ tile_hist /* two-pass sort: [batch][SEG][tiles * NWIN], or nullptr */) {
    __shared__ uint32_t h[NBUCKET];
    uint32_t m = blockIdx.z, w = blockIdx.y;
    uint32_t n = bd.n[m];
    uint32_t lo = blockIdx.x * SORT_TILE;
    const uint32_t T1 = gridDim.x * NWIN, t1 = w * gridDim.x + blockIdx.x;
    if (lo >= n) {
        if (tile_hist)
            for (uint32_t sgm = threadIdx.x; sgm < SEG; sgm += blockDim.x) tile_hist[((size_t)m * SEG + sgm) * T1 + t1] = 0;
        return;
    }
    uint32_t hi = lo + SORT_TILE < n ? lo + SORT_TILE : n;
    const uint16_t *d = dig + (size_t)m * dig_stride + (size_t)w * n;
    tile_histogram(h, d, lo, hi);
    uint32_t *cnt = count + (size_t)m * NBUCKET;
    // every workgroup flushes from its own offset: 256 of them walking the counters in the same order met at the same addresses
    // (k_hist 36.8 -> 33.1 us on average, profiles/r04_ab_chain_blocks.txt section 5)
    const uint32_t rot = ((blockIdx.y * gridDim.x + blockIdx.x) * 128u) & (NBUCKET - 1);
    for (uint32_t i = threadIdx.x; i < NBUCKET; i += blockDim.x) {      // (r05: two counters per 64-bit atomic change nothing: 35.6 us either way, profiles/r05_ab_misc.txt)
        const uint32_t b = (i + rot) & (NBUCKET - 1);
        uint32_t c = h[b];
        if (c) atomicAdd(&cnt[b], c);
    }
    if (tile_hist) {                       // entries of this tile per segment (= SEG_BUCKETS consecutive buckets)
        for (uint32_t sgm = threadIdx.x; sgm < SEG; sgm += blockDim.x) {
            uint32_t c = 0;
            for (uint32_t b = 0; b < SEG_BUCKETS; ++b) c += h[sgm * SEG_BUCKETS + ((b + sgm) & (SEG_BUCKETS - 1))];   // skewed: no bank conflicts
            tile_hist[((size_t)m * SEG + sgm) * T1 + t1] = c;
        }
    }
}

__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t *total);   // defined with k_plan

// ---- two-pass (MSD) variant of the scatter, for large MSMs -----------------------------------------------------------
// The single-pass k_scatter writes every 4-byte entry to a random place of the whole sorted array (one bucket out of
// 2^15 per entry: a tile holds < 1 entry per bucket, so nothing coalesces and every (tile, bucket) pair costs a global
// atomic) -- 15 % of a 12 * 2^20 witness commit.  Two passes instead:
//   A  k_group   : entries -> SEG = 128 segments of 256 consecutive buckets.  A tile contributes thousands of entries to
//                  each segment, at offsets known from the per-tile segment counts (k_hist) scanned by k_scan_seg: the
//                  writes are long coalesced runs, no global atomics.
//   B  k_scatter2: tiles of the GROUPED array do the bucket-level counting sort.  A tile now touches 1-2 segments, i.e.
//                  a few hundred buckets inside a ~MB region that lives in L2: the random 4-byte writes merge there and
//                  the number of global reservations drops ~40x.
// Within a bucket the order of entries is irrelevant (exact group arithmetic), so neither pass needs to be stable.
__global__ void SRS_KERNEL_BOUNDS(1024, 1)
    k_scan_seg(uint32_t *__restrict__ tile_hist, uint32_t T1, const uint32_t *__restrict__ plan, size_t plan_stride) {
    // grid = (SEG, batch): exclusive scan of the T1 per-tile counts of one segment, offset by the segment's start off[seg * 256]
    __shared__ uint32_t lds[64];
    const uint32_t sgm = blockIdx.x, m = blockIdx.y;
    uint32_t *row = tile_hist + ((size_t)m * SEG + sgm) * T1;
    const uint32_t base = plan[(size_t)m * plan_stride + (size_t)sgm * SEG_BUCKETS];        // plan[0][b] = entry offset of bucket b
    uint32_t carry = 0;
    for (uint32_t at = 0; at < T1; at += blockDim.x) {
        const uint32_t i = at + threadIdx.x;
        const uint32_t v = i < T1 ? row[i] : 0;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(v, lds, &total);
        if (i < T1) row[i] = base + carry + ex;
        carry += total;
    }
}

// r03: both passes go through LDS.  A lane-per-entry global store of the first version met ~50 different cache lines per
// wavefront instruction -- the address path of a CU takes about one line per cycle, so k_group / k_scatter2 ran at ~1/4 of what
// their traffic costs.  Now a workgroup sorts a sub-tile of entries by segment (bucket) inside LDS and copies it out in index
// order: consecutive lanes store consecutive addresses of a run.
constexpr uint32_t GRP_PER = 16, GRP_SUB = SORT_THREADS * GRP_PER;      // digit slots per thread / per sub-tile of k_group
// payload of digit row w, less the scalar's index: the table entry of window w -- for a compact key the entry of window w & 7, marked
// as phi of it for the rows of k2
template <bool COMPACT>
__device__ __forceinline__ uint32_t payload_base(uint32_t w, uint32_t table_stride, uint32_t base) {
    if (COMPACT) return ((w & (NWIN_COMPACT - 1)) * table_stride + base) | (w >= NWIN_COMPACT ? PAY_ENDO : 0u);
    return w * table_stride + base;
}
template <bool COMPACT>
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 1)
    k_group(const uint16_t *__restrict__ dig, size_t dig_stride, BatchDesc bd, const uint32_t *__restrict__ tile_hist,
            uint16_t *__restrict__ gkey, uint32_t *__restrict__ gpay, size_t g_stride, uint32_t table_stride, uint32_t SORT_TILE,
            const uint32_t *__restrict__ plan, size_t plan_stride, uint16_t *__restrict__ tb, size_t tb_stride, uint32_t arr) {
    __shared__ uint32_t cur[SEG], cnt[SEG], lb[SEG], sc[64];
    __shared__ uint32_t spay[GRP_SUB];
    __shared__ uint16_t skey[GRP_SUB];
    const uint32_t m = blockIdx.z, w = blockIdx.y, tid = threadIdx.x;
    if (tb) {
        // slot mode: k_expand's work (the thread -> bucket map of level 0, from the plan array `arr`) rides on this launch, a bucket per
        // wavefront and round -- one dependent launch less per set of a chunked commit (r04)
        const uint32_t *tp = plan + (size_t)m * plan_stride + (size_t)arr * (NBUCKET + 1);
        uint16_t *map = tb + (size_t)m * tb_stride;
        const uint32_t waves = gridDim.x * gridDim.y * (blockDim.x >> 6);
        const uint32_t wv = (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (tid >> 6), lane = tid & 63u;
        for (uint32_t b = wv; b < NBUCKET; b += waves) {
            const uint32_t s = tp[b], e = tp[b + 1];
            for (uint32_t t = s + lane; t < e; t += 64) map[t] = (uint16_t)b;
        }
    }
    const uint32_t n = bd.n[m];
    const uint32_t lo = blockIdx.x * SORT_TILE;
    if (lo >= n) return;
    const uint32_t hi = lo + SORT_TILE < n ? lo + SORT_TILE : n;
    const uint32_t T1 = gridDim.x * NWIN, t1 = w * gridDim.x + blockIdx.x;
    for (uint32_t sgm = tid; sgm < SEG; sgm += blockDim.x) cur[sgm] = tile_hist[((size_t)m * SEG + sgm) * T1 + t1];
    const uint16_t *d = dig + (size_t)m * dig_stride + (size_t)w * n;
    uint16_t *ok = gkey + (size_t)m * g_stride;
    uint32_t *op = gpay + (size_t)m * g_stride;
    const uint32_t pay0 = payload_base<COMPACT>(w, table_stride, bd.base[m]);
    for (uint32_t sub = lo; sub < hi; sub += GRP_SUB) {                 // workgroup-uniform
        for (uint32_t sgm = tid; sgm < SEG; sgm += blockDim.x) cnt[sgm] = 0;
        __syncthreads();
        // the thread's GRP_PER consecutive digit slots (two 16-byte loads when they are aligned and inside the tile)
        const uint32_t i0 = sub + tid * GRP_PER;
        uint32_t code[GRP_PER], rank[GRP_PER];
        if (i0 + GRP_PER <= hi && (reinterpret_cast<uintptr_t>(d + i0) & 15u) == 0) {
            const uint4 *v = reinterpret_cast<const uint4 *>(d + i0);
#pragma unroll
            for (uint32_t q = 0; q < GRP_PER / 8; ++q) {
                const uint4 x = v[q];
                code[8 * q + 0] = x.x & 0xFFFFu; code[8 * q + 1] = x.x >> 16;
                code[8 * q + 2] = x.y & 0xFFFFu; code[8 * q + 3] = x.y >> 16;
                code[8 * q + 4] = x.z & 0xFFFFu; code[8 * q + 5] = x.z >> 16;
                code[8 * q + 6] = x.w & 0xFFFFu; code[8 * q + 7] = x.w >> 16;
            }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < GRP_PER; ++k) code[k] = i0 + k < hi ? (uint32_t)d[i0 + k] : 0xFFFFu;
        }
#pragma unroll
        for (uint32_t k = 0; k < GRP_PER; ++k)
            rank[k] = code[k] != 0xFFFFu ? atomicAdd(&cnt[(code[k] & 0x7FFFu) / SEG_BUCKETS], 1u) : 0u;
        __syncthreads();
        uint32_t n_sub;
        const uint32_t ex = block_exclusive_scan(tid < SEG ? cnt[tid] : 0u, sc, &n_sub);
        if (tid < SEG) lb[tid] = ex;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < GRP_PER; ++k) {
            if (code[k] != 0xFFFFu) {
                const uint32_t bkt = code[k] & 0x7FFFu, pos = lb[bkt / SEG_BUCKETS] + rank[k];
                skey[pos] = (uint16_t)bkt;
                spay[pos] = (pay0 + i0 + k) | ((code[k] & 0x8000u) << 16);
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < n_sub; i += blockDim.x) {             // index order: a segment's run goes out as one contiguous piece
            const uint32_t key = skey[i], sgm = key / SEG_BUCKETS, g = cur[sgm] + (i - lb[sgm]);
            ok[g] = (uint16_t)key;
            op[g] = spay[i];
        }
        __syncthreads();
        if (tid < SEG) cur[tid] += cnt[tid];
    }
}

constexpr uint32_t S2_PER = 8, S2_RANGE = 2 * SEG_BUCKETS;               // entries per thread; buckets a tile may span on the LDS path
static_assert(SORT_TILE2 == SORT_THREADS * S2_PER, "k_scatter2: one tile = S2_PER entries per thread");
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 2)
    k_scatter2(const uint16_t *__restrict__ gkey, const uint32_t *__restrict__ gpay, size_t g_stride,
               const uint32_t *__restrict__ plan, size_t plan_stride, uint32_t *__restrict__ cursor /* [batch][NBUCKET] */,
               uint32_t *__restrict__ sorted, size_t sorted_stride, uint32_t TILE2) {
    __shared__ uint32_t cnt[S2_RANGE], lb[S2_RANGE], gb[S2_RANGE], sc[64];
    __shared__ uint32_t spay[SORT_TILE2];
    __shared__ uint16_t skey[SORT_TILE2];
    const uint32_t m = blockIdx.y, tid = threadIdx.x;
    const uint32_t total = plan[(size_t)m * plan_stride + NBUCKET];        // number of non-zero digits of this MSM
    // XCD-aware tile mapping: workgroups are dealt round-robin to the 8 XCDs (each with its own L2), so workgroup b
    // takes tile (b % 8) * ceil(tiles / 8) + b / 8 -- every XCD sorts one contiguous eighth of the grouped array, i.e.
    // one eighth of the buckets, and the stores to a cache line all come from the same L2 and merge there
    const uint32_t n_tiles = (total + TILE2 - 1) / TILE2, per_xcd = (n_tiles + 7) / 8;
    if (blockIdx.x / 8 >= per_xcd) return;
    const uint32_t tile_id = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (tile_id >= n_tiles) return;
    const uint32_t lo = tile_id * TILE2;
    if (lo >= total) return;
    const uint32_t hi = lo + TILE2 < total ? lo + TILE2 : total;
    const uint16_t *key = gkey + (size_t)m * g_stride;
    const uint32_t *pay = gpay + (size_t)m * g_stride;
    uint32_t *cur = cursor + (size_t)m * NBUCKET;
    uint32_t *out = sorted + (size_t)m * sorted_stride;
    // the grouped array is ordered by segment: this tile only holds buckets of segments seg(first) .. seg(last)
    const uint32_t b_lo = ((uint32_t)key[lo] / SEG_BUCKETS) * SEG_BUCKETS;
    const uint32_t b_hi = ((uint32_t)key[hi - 1] / SEG_BUCKETS + 1) * SEG_BUCKETS;
    if (b_hi - b_lo > S2_RANGE) {            // a tile over more than two segments (few entries for the bucket range): entry by entry
        for (uint32_t i = lo + tid; i < hi; i += blockDim.x) out[atomicAdd(&cur[key[i]], 1u)] = pay[i];
        return;
    }
    for (uint32_t b = tid; b < S2_RANGE; b += blockDim.x) cnt[b] = 0;
    __syncthreads();
    const uint32_t i0 = lo + tid * S2_PER;
    uint32_t kk[S2_PER], pp[S2_PER], rank[S2_PER];
    if (i0 + S2_PER <= hi && (reinterpret_cast<uintptr_t>(key + i0) & 15u) == 0 && (reinterpret_cast<uintptr_t>(pay + i0) & 15u) == 0) {
        const uint4 x = *reinterpret_cast<const uint4 *>(key + i0);
        kk[0] = x.x & 0xFFFFu; kk[1] = x.x >> 16; kk[2] = x.y & 0xFFFFu; kk[3] = x.y >> 16;
        kk[4] = x.z & 0xFFFFu; kk[5] = x.z >> 16; kk[6] = x.w & 0xFFFFu; kk[7] = x.w >> 16;
        const uint4 p0 = *reinterpret_cast<const uint4 *>(pay + i0), p1 = *reinterpret_cast<const uint4 *>(pay + i0 + 4);
        pp[0] = p0.x; pp[1] = p0.y; pp[2] = p0.z; pp[3] = p0.w; pp[4] = p1.x; pp[5] = p1.y; pp[6] = p1.z; pp[7] = p1.w;
    } else {
#pragma unroll
        for (uint32_t k = 0; k < S2_PER; ++k) {
            kk[k] = i0 + k < hi ? (uint32_t)key[i0 + k] : 0xFFFFu;
            pp[k] = i0 + k < hi ? pay[i0 + k] : 0u;
        }
    }
#pragma unroll
    for (uint32_t k = 0; k < S2_PER; ++k) rank[k] = kk[k] != 0xFFFFu ? atomicAdd(&cnt[kk[k] - b_lo], 1u) : 0u;
    __syncthreads();
    uint32_t n_tile;
    const uint32_t c = tid < S2_RANGE ? cnt[tid] : 0u;
    const uint32_t ex = block_exclusive_scan(c, sc, &n_tile);
    if (tid < S2_RANGE) {
        lb[tid] = ex;
        gb[tid] = c ? atomicAdd(&cur[b_lo + tid], c) : 0u;                 // reserve [base, base + c) of the bucket
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < S2_PER; ++k) {
        if (kk[k] != 0xFFFFu) {
            const uint32_t pos = lb[kk[k] - b_lo] + rank[k];
            skey[pos] = (uint16_t)(kk[k] - b_lo);
            spay[pos] = pp[k];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_tile; i += blockDim.x) {
        const uint32_t b = skey[i];
        out[gb[b] + (i - lb[b])] = spay[i];
    }
}

#ifndef SCATTER_RES_INFLIGHT
#define SCATTER_RES_INFLIGHT 4
#endif
template <bool COMPACT>
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 1)
    k_scatter(const uint16_t *__restrict__ dig, size_t dig_stride, BatchDesc bd,
              uint32_t *__restrict__ cursor /* [batch][NBUCKET] */, uint32_t *__restrict__ sorted,
              size_t sorted_stride, uint32_t table_stride, uint32_t SORT_TILE) {
    __shared__ uint32_t h[NBUCKET];
    uint32_t m = blockIdx.z, w = blockIdx.y;
    uint32_t n = bd.n[m];
    uint32_t lo = blockIdx.x * SORT_TILE;
    if (lo >= n) return;
    uint32_t hi = lo + SORT_TILE < n ? lo + SORT_TILE : n;
    const uint16_t *d = dig + (size_t)m * dig_stride + (size_t)w * n;
    tile_histogram(h, d, lo, hi);
    uint32_t *cur = cursor + (size_t)m * NBUCKET;
    // the reservations are returning device-scope atomics: RES in flight per thread (32 = all of a thread's buckets in one round
    // measured no faster, r03: the kernel waits for its scattered 4-byte stores, profiles/r03_sq_counters_msm.txt)
    constexpr int RES = SCATTER_RES_INFLIGHT;
    for (uint32_t b0 = threadIdx.x; b0 < NBUCKET; b0 += RES * blockDim.x) {
        uint32_t c[RES], r[RES];
#pragma unroll
        for (int u = 0; u < RES; ++u) c[u] = b0 + u * blockDim.x < NBUCKET ? h[b0 + u * blockDim.x] : 0u;
#pragma unroll
        for (int u = 0; u < RES; ++u) r[u] = c[u] ? atomicAdd(&cur[b0 + u * blockDim.x], c[u]) : 0u;   // reserve [base, base+c)
#pragma unroll
        for (int u = 0; u < RES; ++u) if (c[u]) h[b0 + u * blockDim.x] = r[u];
    }
    __syncthreads();
    uint32_t *out = sorted + (size_t)m * sorted_stride;
    const uint32_t pay0 = payload_base<COMPACT>(w, table_stride, bd.base[m]);
    for_each_digit(d, lo, hi, [&](uint32_t i, uint32_t code) {
        if (code != 0xFFFFu) {
            uint32_t pos = atomicAdd(&h[code & 0x7FFFu], 1u);
            out[pos] = (pay0 + i) | ((code & 0x8000u) << 16);
        }
    });
}

// Wide windows: the NSEG_W virtual MSMs share ONE parts / map array per level parity instead of a worst-case stride each
// (a witness of small values puts every entry into segment 0).  base[l][v] = first level-l part of segment v in the flat
// thread space of level l (base[l][NSEG_W] = their number); in memory the parts of level l of segment v start at
// base[l & 1][v] of ping (even l) / pong (odd l): a level never has more parts than the level two below it.
// NS: the segment capacity.  NSEG_W for the wide flow and the single plain MSM; the batched plain flow links up to PLAIN_BATCH_SEG
// segments, the (member, window) pairs of a set.  Every kernel that reads a link or the tile spaces of k_seg_scan carries NS with
// NSEG_W as its default, so what the 16-segment flows launch is compiled as before and the batched flow has instantiations of its own.
constexpr uint32_t PLAIN_BATCH_SEG = BATCH_ARGS * NWIN;      // 256
template <uint32_t NS = NSEG_W>
struct LinkT {
    uint32_t base[MAX_LEVELS + 1][NS + 1];
};
using Link = LinkT<>;
template <uint32_t NS = NSEG_W>
__device__ __forceinline__ uint32_t link_segment(const uint32_t *__restrict__ base, uint32_t t) {   // base[v] <= t < base[v + 1]
    if constexpr (NS == NSEG_W) {
        uint32_t v = 0;
#pragma unroll
        for (uint32_t u = 1; u < NSEG_W; ++u) v += (t >= base[u]) ? 1u : 0u;
        return v;
    } else {                                  // largest v in [0, NS) with base[v] <= t (base is non-decreasing, base[0] = 0): log2(NS) loads
        uint32_t lo = 0, hi = NS;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (base[mid] <= t) lo = mid; else hi = mid;
        }
        return lo;
    }
}

// ---------------------------------------------------------------------------------------------
// 2b. wide windows: scalars -> 13 signed 20-bit digits -> entries grouped by segment (the top 4 bits of the bucket)
// code = 0xFFFFFFFF (zero digit) | (|d| - 1) [19 bits] | sign << 31
// ---------------------------------------------------------------------------------------------
struct WideDesc {
    const fe_t *ptr;
    uint32_t n, base;               // scalars, first base inside the key
    uint32_t rank, world;           // as k_digits
    int is_mont;
};

// digit rows per scalar of the wide flow: 13 windows of the scalar, or (compact key) 7 of |k1| then 7 of |k2|
constexpr int wide_digits(bool compact) { return compact ? 2 * NWIN_WC : NWIN_W; }

template <class C, bool COMPACT>
__device__ __forceinline__ void wide_codes(const WideDesc &wd, uint32_t i, uint32_t (&code)[wide_digits(COMPACT)]) {
    using S = typename C::S;
    if (i >= wd.n) {
#pragma unroll
        for (int w = 0; w < wide_digits(COMPACT); ++w) code[w] = 0xFFFFFFFFu;
        return;
    }
    fe_t s = wd.ptr[Stripes{wd.rank, wd.world}.global_index((size_t)i)];
    if (wd.is_mont) s = S::from_mont(s);
    if constexpr (COMPACT) {                  // k = k1 + lambda k2: rows 0..6 from |k1|, rows 7..13 from |k2| (entries of phi(P), see k_seg_pass)
        const glv_t g = glv_decompose<C>(s);
        const auto put = [&](int w, uint32_t mag, bool minus) { code[w] = mag ? ((mag - 1u) | (minus ? 0x80000000u : 0u)) : 0xFFFFFFFFu; };
        recode_half<WBITS_W, NWIN_WC>(g.k1, g.neg1, put);
        recode_half<WBITS_W, NWIN_WC>(g.k2, g.neg2, [&](int w, uint32_t mag, bool minus) { put(NWIN_WC + w, mag, minus); });
        return;
    }
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < NWIN_W; ++w) {
        const int bit = WBITS_W * w, limb = bit >> 5, sh = bit & 31;
        uint64_t two = s.v[limb];
        if (limb + 1 < 8) two |= (uint64_t)s.v[limb + 1] << 32;
        const uint32_t v = ((uint32_t)(two >> sh) & 0xFFFFFu) + carry;
        if (v > 0x80000u) {
            code[w] = ((0x100000u - v) - 1u) | 0x80000000u;   // negative digit, magnitude 1..0x7FFFF (v = 2^20: zero digit, carry)
            carry = 1;
        } else {
            code[w] = v ? (v - 1u) : 0xFFFFFFFFu;             // positive digit 1..0x80000, or zero
            carry = 0;
        }
    }
}

// plain keys: the NWIN signed 16-bit digits of k_digits, in the 32-bit code format above -- code[w] is the entry of WINDOW w, its bucket the
// low 15 bits.  v = 2^16 (0xFFFF + carry) leaves magnitude 0, a zero digit that carries; the top window never carries out (scalars < 2^254).
template <class C>
__device__ __forceinline__ void plain_codes(const WideDesc &wd, uint32_t i, uint32_t (&code)[NWIN]) {
    using S = typename C::S;
    if (i >= wd.n) {
#pragma unroll
        for (int w = 0; w < NWIN; ++w) code[w] = 0xFFFFFFFFu;
        return;
    }
    fe_t s = wd.ptr[Stripes{wd.rank, wd.world}.global_index((size_t)i)];
    if (wd.is_mont) s = S::from_mont(s);
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < NWIN; ++w) {
        const uint32_t v = ((s.v[w >> 1] >> ((w & 1) * 16)) & 0xFFFFu) + carry;
        if (v > 0x8000u) {
            code[w] = ((0x10000u - v) - 1u) | 0x80000000u;    // negative digit, magnitude 1..0x7FFF (v = 2^16: 0xFFFFFFFF, the zero digit)
            carry = 1;
        } else {
            code[w] = v ? (v - 1u) : 0xFFFFFFFFu;             // positive digit 1..0x8000, or zero
            carry = 0;
        }
    }
}

// plain keys of form 2 (msm_plain = 2): k = k1 + lambda k2 (glv.cuh), rows 0..7 the 8 signed 16-bit digits of k1, rows 8..15 those of k2,
// in the same 32-bit code format.  Row r is an entry of WINDOW r % 8 -- phi is a homomorphism, so digit w of k2 weighs 2^(16 w) phi(P) --
// and rows 8..15 gather phi of the base (k_seg_pass flags them PAY_ENDO).  The top window of a half never carries out: the bound
// compact keys rely on for their 8 narrow windows (recode_half above: |k1|, |k2| < 2^126 by tools/gen_glv_consts.py, so the eighth
// window of a half holds at most 14 bits plus the carry; the split itself is glv_decompose, glv.cuh).
template <class C>
__device__ __forceinline__ void plain_glv_codes(const WideDesc &wd, uint32_t i, uint32_t (&code)[NWIN]) {
    using S = typename C::S;
    static_assert(2 * NWIN_COMPACT == NWIN, "two halves of 8 windows fill the 16 digit rows");
    if (i >= wd.n) {
#pragma unroll
        for (int w = 0; w < NWIN; ++w) code[w] = 0xFFFFFFFFu;
        return;
    }
    fe_t s = wd.ptr[Stripes{wd.rank, wd.world}.global_index((size_t)i)];
    if (wd.is_mont) s = S::from_mont(s);
    const glv_t g = glv_decompose<C>(s);
    const auto put = [&](int w, uint32_t mag, bool minus) { code[w] = mag ? ((mag - 1u) | (minus ? 0x80000000u : 0u)) : 0xFFFFFFFFu; };
    recode_half<WBITS, NWIN_COMPACT>(g.k1, g.neg1, put);
    recode_half<WBITS, NWIN_COMPACT>(g.k2, g.neg2, [&](int w, uint32_t mag, bool minus) { put(NWIN_COMPACT + w, mag, minus); });
}

// atomicAdd(ctr, 1) for the lanes with `on` set when they all name the SAME LDS counter: one atomic per wavefront (the leader reserves
// the wavefront's slots, a lane's slot follows from the lanes below it) instead of up to 64 serialised ones.  Wave-uniform control flow
// only.  Returns the lane's slot (meaningless where !on).  For the hot top windows of a compact key's wide flow (msm.h NWIN_WC).
__device__ __forceinline__ uint32_t wave_take(uint32_t *ctr, bool on) {
    const unsigned long long m = __ballot(on ? 1 : 0);
    if (m == 0) return 0u;
    const uint32_t lane = threadIdx.x & 63u;
    const int leader = __ffsll(m) - 1;
    uint32_t first = 0;
    if ((int)lane == leader) first = atomicAdd(ctr, (uint32_t)__popcll(m));
    first = __shfl(first, leader, 64);
    return first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// The two segment passes over the scalars (the digits are recomputed rather than stored: 32 B read per scalar instead of
// 52 B written and read).  A workgroup takes WIDE_TILE scalars = up to 6656 entries (7168 on a compact key); the 16 segment counters are kept per
// wavefront in LDS (64 words = 64 banks), so an atomic only meets the lanes of its own wavefront.
//   GROUP = false: tile_cnt[v][tile] = entries of the tile in segment v; seg_total[v] += the same
//   GROUP = true : tile_cnt holds the scanned offsets (k_seg_scan): the tile's entries are ordered by segment in LDS (the
//                  returning atomic is the entry's rank) and leave as 16 coalesced runs of
//                  (key = low 15 bits of the bucket, payload = table index | sign << 31)
// COMPACT (a compact key with the 7-window table, msm.h): 14 digit rows, row w gathers window w % 7 and rows 7..13 carry PAY_ENDO -- the
// staging is sized from the digit count (512 x 14 entries, 43 KB).  Instantiations of their own: what full keys launch is compiled as before.
// PLAIN (a plain key, msm.h): the 16 signed 16-bit digits of plain_codes, and the segment of an entry is its WINDOW -- the same for every
// lane, so each counter is taken once per wavefront (wave_take); every entry gathers window 0, payload = base index | sign << 31
// (512 x 16 entries, 48 KB of staging).
// PLAIN with GLV (a plain key of form 2): the 16 rows of plain_glv_codes; the segment of row r is the window r % 8, still the same for every
// lane, so a window's counter is taken twice per scalar; rows 8..15 carry PAY_ENDO (the base index stays below bit 30: keys are <= 2^27
// bases).  Segments 8..15 stay empty.  The same staging.
template <class C, bool GROUP, bool COMPACT, bool PLAIN = false, bool GLV = false>
__global__ void SRS_KERNEL_BOUNDS(WIDE_THREADS, 1)
    k_seg_pass(WideDesc wd, uint32_t *__restrict__ tile_cnt, uint32_t T, uint32_t *__restrict__ seg_total,
               uint16_t *__restrict__ gkey, uint32_t *__restrict__ gpay, uint32_t table_stride) {
    static_assert(!(PLAIN && COMPACT) && NWIN == (int)NSEG_W, "a plain key's windows are the segments");
    static_assert(PLAIN || !GLV, "GLV selects the second form of a plain key");
    constexpr int ND = PLAIN ? NWIN : wide_digits(COMPACT);
    constexpr uint32_t NW = WIDE_THREADS / 64, STAGE = GROUP ? WIDE_TILE * ND : 1;
    __shared__ uint32_t wc[NW][NSEG_W];          // counts, then (GROUP) the next free staging slot of (wavefront, segment)
    __shared__ uint32_t ss[NSEG_W + 1], goff[NSEG_W];
    __shared__ uint16_t skey[STAGE];
    __shared__ uint32_t spay[STAGE];
    const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6;
    if (threadIdx.x < NW * NSEG_W) (&wc[0][0])[threadIdx.x] = 0;
    uint32_t code[WIDE_PER][ND];
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
        const uint32_t i = tile * WIDE_TILE + k * WIDE_THREADS + threadIdx.x;
        if constexpr (PLAIN && GLV) plain_glv_codes<C>(wd, i, code[k]);
        else if constexpr (PLAIN) plain_codes<C>(wd, i, code[k]); else wide_codes<C, COMPACT>(wd, i, code[k]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
#pragma unroll
        for (int w = 0; w < ND; ++w) {
            const uint32_t c = code[k][w];
            if (PLAIN) {                                      // segment = window: one counter for the whole wavefront
                wave_take(&wc[wave][GLV ? w % NWIN_COMPACT : w], c != 0xFFFFFFFFu);
                continue;
            }
            if (COMPACT && (w + 1) % NWIN_WC == 0) {          // a half's top digit is <= 2^6: always segment 0, from every lane
                wave_take(&wc[wave][0], c != 0xFFFFFFFFu);
                continue;
            }
            if (c != 0xFFFFFFFFu) atomicAdd(&wc[wave][(c >> 15) & (NSEG_W - 1)], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < NSEG_W) {
        const uint32_t v = threadIdx.x;
        uint32_t tot = 0;
        for (uint32_t w = 0; w < NW; ++w) tot += wc[w][v];
        if (!GROUP) {
            tile_cnt[(size_t)v * T + tile] = tot;
            if (tot) atomicAdd(&seg_total[v], tot);
        } else {
            ss[v + 1] = tot;
            goff[v] = tile_cnt[(size_t)v * T + tile];
        }
    }
    if (!GROUP) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t v = 0; v < NSEG_W; ++v) {
            const uint32_t c = ss[v + 1];
            ss[v] = run;
            run += c;
        }
        ss[NSEG_W] = run;
    }
    __syncthreads();
    if (threadIdx.x < NSEG_W) {                  // counts -> first staging slot of (wavefront, segment)
        const uint32_t v = threadIdx.x;
        uint32_t run = ss[v];
        for (uint32_t w = 0; w < NW; ++w) {
            const uint32_t c = wc[w][v];
            wc[w][v] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
        const uint32_t i = tile * WIDE_TILE + k * WIDE_THREADS + threadIdx.x;
#pragma unroll
        for (int w = 0; w < ND; ++w) {
            const uint32_t c = code[k][w];
            const bool top = PLAIN || (COMPACT && (w + 1) % NWIN_WC == 0);
            const uint32_t pos_top = top ? wave_take(&wc[wave][PLAIN ? (GLV ? w % NWIN_COMPACT : w) : 0], c != 0xFFFFFFFFu) : 0u;
            if (c != 0xFFFFFFFFu) {
                const uint32_t pos = top ? pos_top : atomicAdd(&wc[wave][(c >> 15) & (NSEG_W - 1)], 1u);
                skey[pos] = (uint16_t)(c & 0x7FFFu);
                const uint32_t row = PLAIN ? wd.base | (GLV && w >= NWIN_COMPACT ? PAY_ENDO : 0u)
                                   : COMPACT ? ((uint32_t)w % NWIN_WC * table_stride + wd.base) | (w >= NWIN_WC ? PAY_ENDO : 0u)
                                             : (uint32_t)w * table_stride + wd.base;
                spay[pos] = (row + i) | (c & 0x80000000u);
            }
        }
    }
    __syncthreads();
    for (uint32_t v = 0; v < NSEG_W; ++v) {
        const uint32_t lo = ss[v], hi = ss[v + 1], g0 = goff[v];
        for (uint32_t e = lo + threadIdx.x; e < hi; e += WIDE_THREADS) {
            gkey[g0 + (e - lo)] = skey[e];
            gpay[g0 + (e - lo)] = spay[e];
        }
    }
}

// The segment passes of a BATCH of MSMs on a plain key (the batched plain flow, host driver): the segment is the pair (member, window).
// The descriptor travels as a kernel argument, like BatchDesc: the non-empty members of the set, packed; tile0[j] = first workgroup of
// member j in the flat tile space (tile0[j] = T from the member count on), so a workgroup's WIDE_TILE scalars belong to ONE member.
struct PlainBatchDesc {
    const fe_t *ptr[BATCH_ARGS];
    uint32_t n[BATCH_ARGS];
    uint32_t base[BATCH_ARGS];
    uint32_t tile0[BATCH_ARGS + 1];
    int is_mont;
};
// Inside the workgroup this is k_seg_pass<PLAIN (, GLV)>: the member's windows are the 16 (8) per-wavefront LDS counters, each taken
// once (twice) per wavefront and scalar; 48 KB of staging.  The global segment of window w is j * windows + w: row (segment) of
// tile_cnt [segments][T], zeroed by the host -- a row only holds counts at its own member's tiles.  Payloads are those of the single
// MSM (base[j] + i | sign << 31, | PAY_ENDO for the rows of k2), so level 0 is k_accum0 / k_accum0c unchanged.
template <class C, bool GROUP, bool GLV>
__global__ void SRS_KERNEL_BOUNDS(WIDE_THREADS, 1)
    k_seg_pass_b(PlainBatchDesc bd, uint32_t *__restrict__ tile_cnt, uint32_t T, uint32_t *__restrict__ seg_total,
                 uint16_t *__restrict__ gkey, uint32_t *__restrict__ gpay) {
    constexpr int ND = NWIN;
    constexpr uint32_t NWN = GLV ? NWIN_COMPACT : NWIN;          // windows = segments of a member
    constexpr uint32_t NW = WIDE_THREADS / 64, STAGE = GROUP ? WIDE_TILE * ND : 1;
    __shared__ uint32_t wc[NW][NWIN];
    __shared__ uint32_t ss[NWIN + 1], goff[NWIN];
    __shared__ uint16_t skey[STAGE];
    __shared__ uint32_t spay[STAGE];
    const uint32_t tile = blockIdx.x, wave = threadIdx.x >> 6;
    uint32_t j = 0;                                               // the tile's member (workgroup-uniform)
#pragma unroll
    for (uint32_t u = 1; u < BATCH_ARGS; ++u) j += (tile >= bd.tile0[u]) ? 1u : 0u;
    const WideDesc wd{bd.ptr[j], bd.n[j], bd.base[j], 0u, 1u, bd.is_mont};
    const uint32_t mtile = tile - bd.tile0[j];
    const size_t row0 = (size_t)j * NWN;                          // the member's first segment
    if (threadIdx.x < NW * NWIN) (&wc[0][0])[threadIdx.x] = 0;
    uint32_t code[WIDE_PER][ND];
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
        const uint32_t i = mtile * WIDE_TILE + k * WIDE_THREADS + threadIdx.x;
        if constexpr (GLV) plain_glv_codes<C>(wd, i, code[k]); else plain_codes<C>(wd, i, code[k]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
#pragma unroll
        for (int w = 0; w < ND; ++w) wave_take(&wc[wave][GLV ? w % NWIN_COMPACT : w], code[k][w] != 0xFFFFFFFFu);
    }
    __syncthreads();
    if (threadIdx.x < NWN) {
        const uint32_t v = threadIdx.x;
        uint32_t tot = 0;
        for (uint32_t w = 0; w < NW; ++w) tot += wc[w][v];
        if (!GROUP) {
            tile_cnt[(row0 + v) * T + tile] = tot;
            if (tot) atomicAdd(&seg_total[row0 + v], tot);
        } else {
            ss[v + 1] = tot;
            goff[v] = tile_cnt[(row0 + v) * T + tile];
        }
    }
    if (!GROUP) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t run = 0;
        for (uint32_t v = 0; v < NWN; ++v) {
            const uint32_t c = ss[v + 1];
            ss[v] = run;
            run += c;
        }
        ss[NWN] = run;
    }
    __syncthreads();
    if (threadIdx.x < NWN) {                     // counts -> first staging slot of (wavefront, window)
        const uint32_t v = threadIdx.x;
        uint32_t run = ss[v];
        for (uint32_t w = 0; w < NW; ++w) {
            const uint32_t c = wc[w][v];
            wc[w][v] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < WIDE_PER; ++k) {
        const uint32_t i = mtile * WIDE_TILE + k * WIDE_THREADS + threadIdx.x;
#pragma unroll
        for (int w = 0; w < ND; ++w) {
            const uint32_t c = code[k][w];
            const uint32_t pos = wave_take(&wc[wave][GLV ? w % NWIN_COMPACT : w], c != 0xFFFFFFFFu);
            if (c != 0xFFFFFFFFu) {              // (a staging slot below WIDE_TILE * ND: a tile holds at most that many entries)
                skey[pos] = (uint16_t)(c & 0x7FFFu);
                spay[pos] = ((wd.base | (GLV && w >= NWIN_COMPACT ? PAY_ENDO : 0u)) + i) | (c & 0x80000000u);
            }
        }
    }
    __syncthreads();
    for (uint32_t v = 0; v < NWN; ++v) {
        const uint32_t lo = ss[v], hi = ss[v + 1], g0 = goff[v];
        for (uint32_t e = lo + threadIdx.x; e < hi; e += WIDE_THREADS) {
            gkey[g0 + (e - lo)] = skey[e];
            gpay[g0 + (e - lo)] = spay[e];
        }
    }
}

// grid = the segments in use (the 16-segment flows: NSEG_W): block v turns row v of tile_cnt into exclusive offsets into the grouped
// arrays (segment v starts where the totals of segments < v end).  Block 0 also leaves seg_off[0..NS] and the tile space of the
// per-segment counting sort: tile_base[v] = first workgroup of segment v when every segment is cut into tiles of `tile_g` entries.
// The tile size aims at SORT_TARGET_BLOCKS - NSEG_W full tiles whatever NS; every segment with entries adds a partly filled one, so
// k_hist_g / k_group_g need SORT_TARGET_BLOCKS - NSEG_W + (segments in use) workgroups.
template <uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(1024, 1)
    k_seg_scan(uint32_t *__restrict__ tile_cnt, uint32_t T, const uint32_t *__restrict__ seg_total, uint32_t *__restrict__ seg_off,
               uint32_t *__restrict__ tile_base /* [NS + 1], then the tile size */,
               uint32_t *__restrict__ tile_base2 /* [NS + 1]: the same for the tiles of k_scatter2_g, then their size */,
               uint32_t small_tiles /* the launch of k_scatter2_g is sized for tiles of SORT_TILE2 / 4 (sets that may be sparse) */) {
    __shared__ uint32_t lds[64];
    const uint32_t v = blockIdx.x;
    uint32_t base = 0;
    for (uint32_t u = 0; u < v; ++u) base += seg_total[u];
    if (v == 0 && threadIdx.x == 0) {
        // tile size from the ACTUAL number of entries (zero digits are gone): <= SORT_TARGET_BLOCKS workgroups of 128 KiB LDS,
        // i.e. one round over the CUs, whatever the share of zeros
        uint32_t all = 0;
        for (uint32_t u = 0; u < NS; ++u) all += seg_total[u];
        uint32_t tile_g = (all + (SORT_TARGET_BLOCKS - NSEG_W) - 1) / (SORT_TARGET_BLOCKS - NSEG_W);
        tile_g = (tile_g + 1023u) & ~1023u;
        if (tile_g < SORT_TILE_MIN) tile_g = SORT_TILE_MIN;
        tile_base[NS + 1] = tile_g;
        uint32_t run = 0, tr = 0;
        for (uint32_t u = 0; u < NS; ++u) {
            seg_off[u] = run;
            tile_base[u] = tr;
            run += seg_total[u];
            tr += (seg_total[u] + tile_g - 1) / tile_g;
        }
        seg_off[NS] = run;
        tile_base[NS] = tr;
        // k_scatter2_g sorts a tile inside LDS only when it spans <= 2 sub-segments (S2_RANGE buckets); with < ~40 entries per bucket a tile
        // of SORT_TILE2 entries spans more and would go entry by entry through global atomics (the sets of a chunked commit, r05): smaller tiles
        const uint32_t tile2 = (small_tiles && all / ((NS == NSEG_W ? NSEG_W : gridDim.x) * NBUCKET) < 40u) ? SORT_TILE2 / 4 : SORT_TILE2;
        uint32_t t2 = 0;
        for (uint32_t u = 0; u < NS; ++u) {
            tile_base2[u] = t2;
            t2 += (seg_total[u] + tile2 - 1) / tile2;
        }
        tile_base2[NS] = t2;
        tile_base2[NS + 1] = tile2;
    }
    uint32_t *row = tile_cnt + (size_t)v * T;
    uint32_t carry = 0;
    for (uint32_t at = 0; at < T; at += blockDim.x) {
        const uint32_t i = at + threadIdx.x;
        const uint32_t c = i < T ? row[i] : 0;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(c, lds, &total);
        if (i < T) row[i] = base + carry + ex;
        carry += total;
    }
}

// counting sort inside the segments, from the grouped (key, payload) arrays: same LDS histogram as k_hist / k_scatter,
// one workgroup per tile of the flat tile space (tile_base)
template <uint32_t NS = NSEG_W>
__device__ __forceinline__ bool wide_tile(const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ tile_base,
                                          uint32_t &v, uint32_t &lo, uint32_t &hi) {
    if (blockIdx.x >= tile_base[NS]) return false;
    const uint32_t tile_g = tile_base[NS + 1];
    v = link_segment<NS>(tile_base, blockIdx.x);
    lo = seg_off[v] + (blockIdx.x - tile_base[v]) * tile_g;
    hi = seg_off[v + 1];
    if (hi > lo + tile_g) hi = lo + tile_g;
    return true;
}

template <uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 1)
    k_hist_g(const uint16_t *__restrict__ gkey, const uint32_t *__restrict__ seg_off, const uint32_t *__restrict__ tile_base,
             uint32_t *__restrict__ count /* [NSEG_W][NBUCKET] */, uint32_t *__restrict__ tile_hist /* [SEG][gridDim.x] or nullptr */) {
    __shared__ uint32_t h[NBUCKET];
    uint32_t v, lo, hi;
    if (!wide_tile<NS>(seg_off, tile_base, v, lo, hi)) return;
    tile_histogram(h, gkey, lo, hi);
    uint32_t *cnt = count + (size_t)v * NBUCKET;
    for (uint32_t b = threadIdx.x; b < NBUCKET; b += blockDim.x) {
        uint32_t c = h[b];
        if (c) atomicAdd(&cnt[b], c);
    }
    if (tile_hist) {                       // entries of this tile per sub-segment (= SEG_BUCKETS consecutive buckets of its segment)
        for (uint32_t sgm = threadIdx.x; sgm < SEG; sgm += blockDim.x) {
            uint32_t c = 0;
            for (uint32_t b = 0; b < SEG_BUCKETS; ++b) c += h[sgm * SEG_BUCKETS + ((b + sgm) & (SEG_BUCKETS - 1))];
            tile_hist[(size_t)sgm * gridDim.x + blockIdx.x] = c;
        }
    }
}

// ---- the wide pipeline's counting sort in two passes through LDS (r03; the narrow pipeline's k_group / k_scatter2 on the grouped pairs of a
// segment): k_scan_seg_g turns the per-tile sub-segment counts into offsets, k_group_g sorts sub-tiles of a tile's pairs by sub-segment
// inside LDS and copies the runs out, k_scatter2_g sorts 8192-entry tiles of a segment by bucket inside LDS.
__global__ void SRS_KERNEL_BOUNDS(1024, 1)
    k_scan_seg_g(uint32_t *__restrict__ tile_hist, uint32_t TG, const uint32_t *__restrict__ tile_base, const uint32_t *__restrict__ plan,
                 size_t plan_stride) {
    // grid = (SEG, NSEG_W): the tiles of segment v are the workgroups tile_base[v] .. tile_base[v + 1] of k_hist_g
    __shared__ uint32_t lds[64];
    const uint32_t sgm = blockIdx.x, v = blockIdx.y;
    const uint32_t t0 = tile_base[v], t1 = tile_base[v + 1];
    uint32_t *row = tile_hist + (size_t)sgm * TG;
    const uint32_t base = plan[(size_t)v * plan_stride + (size_t)sgm * SEG_BUCKETS];        // absolute entry offset of the sub-segment's first bucket
    uint32_t carry = 0;
    for (uint32_t at = t0; at < t1; at += blockDim.x) {                                     // workgroup-uniform
        const uint32_t i = at + threadIdx.x;
        const uint32_t c = i < t1 ? row[i] : 0;
        uint32_t total;
        const uint32_t ex = block_exclusive_scan(c, lds, &total);
        if (i < t1) row[i] = base + carry + ex;
        carry += total;
    }
}

// HOT0 (compact keys): sub-segment 0 of segment 0 holds the two top digit rows -- 1/7 of ALL entries, 3/4 of that segment's: its
// counter is taken once per wavefront (wave_take).  An instantiation of its own; full keys launch k_group_g<false>, compiled as before.
template <bool HOT0, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 1)
    k_group_g(const uint16_t *__restrict__ gkey, const uint32_t *__restrict__ gpay, const uint32_t *__restrict__ seg_off,
              const uint32_t *__restrict__ tile_base, const uint32_t *__restrict__ tile_hist, uint16_t *__restrict__ gkey2,
              uint32_t *__restrict__ gpay2) {
    __shared__ uint32_t cur[SEG], cnt[SEG], lb[SEG], sc[64];
    __shared__ uint32_t spay[GRP_SUB];
    __shared__ uint16_t skey[GRP_SUB];
    const uint32_t tid = threadIdx.x;
    uint32_t v, lo, hi;
    if (!wide_tile<NS>(seg_off, tile_base, v, lo, hi)) return;
    for (uint32_t sgm = tid; sgm < SEG; sgm += blockDim.x) cur[sgm] = tile_hist[(size_t)sgm * gridDim.x + blockIdx.x];
    for (uint32_t sub = lo; sub < hi; sub += GRP_SUB) {                 // workgroup-uniform
        for (uint32_t sgm = tid; sgm < SEG; sgm += blockDim.x) cnt[sgm] = 0;
        __syncthreads();
        uint32_t key[GRP_PER], pay[GRP_PER], rank[GRP_PER];
#pragma unroll
        for (uint32_t k = 0; k < GRP_PER; ++k) {                        // lane-consecutive entries: coalesced 2- and 4-byte loads
            const uint32_t i = sub + k * SORT_THREADS + tid;
            key[k] = i < hi ? (uint32_t)gkey[i] : 0xFFFFu;
            pay[k] = i < hi ? gpay[i] : 0u;
        }
#pragma unroll
        for (uint32_t k = 0; k < GRP_PER; ++k) {
            if (HOT0 && v == 0) {                                       // workgroup-uniform
                const bool hot = key[k] < SEG_BUCKETS;                  // (a padding key is 0xFFFF)
                const uint32_t r = wave_take(&cnt[0], hot);
                rank[k] = hot ? r : key[k] != 0xFFFFu ? atomicAdd(&cnt[key[k] / SEG_BUCKETS], 1u) : 0u;
            } else {
                rank[k] = key[k] != 0xFFFFu ? atomicAdd(&cnt[key[k] / SEG_BUCKETS], 1u) : 0u;
            }
        }
        __syncthreads();
        uint32_t n_sub;
        const uint32_t ex = block_exclusive_scan(tid < SEG ? cnt[tid] : 0u, sc, &n_sub);
        if (tid < SEG) lb[tid] = ex;
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < GRP_PER; ++k) {
            if (key[k] != 0xFFFFu) {
                const uint32_t pos = lb[key[k] / SEG_BUCKETS] + rank[k];
                skey[pos] = (uint16_t)key[k];
                spay[pos] = pay[k];
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < n_sub; i += blockDim.x) {
            const uint32_t kk = skey[i], sgm = kk / SEG_BUCKETS, g = cur[sgm] + (i - lb[sgm]);
            gkey2[g] = (uint16_t)kk;
            gpay2[g] = spay[i];
        }
        __syncthreads();
        if (tid < SEG) cur[tid] += cnt[tid];
    }
}

template <uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(SORT_THREADS, 2)
    k_scatter2_g(const uint16_t *__restrict__ gkey2, const uint32_t *__restrict__ gpay2, const uint32_t *__restrict__ seg_off,
                 const uint32_t *__restrict__ tile_base2, uint32_t *__restrict__ cursor /* [NSEG_W][NBUCKET], absolute */,
                 uint32_t *__restrict__ sorted) {
    __shared__ uint32_t cnt[S2_RANGE], lb[S2_RANGE], gb[S2_RANGE], sc[64];
    __shared__ uint32_t spay[SORT_TILE2];
    __shared__ uint16_t skey[SORT_TILE2];
    const uint32_t tid = threadIdx.x;
    // XCD-aware tile mapping as in k_scatter2: every XCD sorts one contiguous eighth of the flat tile space
    const uint32_t n_tiles = tile_base2[NS], per_xcd = (n_tiles + 7) / 8;
    if (blockIdx.x / 8 >= per_xcd) return;
    const uint32_t tile_id = (blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (tile_id >= n_tiles) return;
    const uint32_t v = link_segment<NS>(tile_base2, tile_id), tile2 = tile_base2[NS + 1];
    const uint32_t lo = seg_off[v] + (tile_id - tile_base2[v]) * tile2;
    const uint32_t hi = lo + tile2 < seg_off[v + 1] ? lo + tile2 : seg_off[v + 1];
    if (lo >= hi) return;
    uint32_t *cur = cursor + (size_t)v * NBUCKET;
    // the grouped array of a segment is ordered by sub-segment: this tile only holds buckets of sub-segments seg(first) .. seg(last)
    const uint32_t b_lo = ((uint32_t)gkey2[lo] / SEG_BUCKETS) * SEG_BUCKETS;
    const uint32_t b_hi = ((uint32_t)gkey2[hi - 1] / SEG_BUCKETS + 1) * SEG_BUCKETS;
    if (b_hi - b_lo > S2_RANGE) {            // a tile over more than two sub-segments (few entries for the bucket range): entry by entry
        for (uint32_t i = lo + tid; i < hi; i += blockDim.x) sorted[atomicAdd(&cur[gkey2[i]], 1u)] = gpay2[i];
        return;
    }
    for (uint32_t b = tid; b < S2_RANGE; b += blockDim.x) cnt[b] = 0;
    __syncthreads();
    uint32_t kk[S2_PER], pp[S2_PER], rank[S2_PER];
#pragma unroll
    for (uint32_t k = 0; k < S2_PER; ++k) {
        const uint32_t i = lo + k * SORT_THREADS + tid;
        kk[k] = i < hi ? (uint32_t)gkey2[i] : 0xFFFFu;
        pp[k] = i < hi ? gpay2[i] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < S2_PER; ++k) rank[k] = kk[k] != 0xFFFFu ? atomicAdd(&cnt[kk[k] - b_lo], 1u) : 0u;
    __syncthreads();
    uint32_t n_tile;
    const uint32_t c = tid < S2_RANGE ? cnt[tid] : 0u;
    const uint32_t ex = block_exclusive_scan(c, sc, &n_tile);
    if (tid < S2_RANGE) {
        lb[tid] = ex;
        gb[tid] = c ? atomicAdd(&cur[b_lo + tid], c) : 0u;                 // reserve [base, base + c) of the bucket (absolute)
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < S2_PER; ++k) {
        if (kk[k] != 0xFFFFu) {
            const uint32_t pos = lb[kk[k] - b_lo] + rank[k];
            skey[pos] = (uint16_t)(kk[k] - b_lo);
            spay[pos] = pp[k];
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < n_tile; i += blockDim.x) {
        const uint32_t b = skey[i];
        sorted[gb[b] + (i - lb[b])] = spay[i];
    }
}

// ---------------------------------------------------------------------------------------------
// 3. plan: bucket offsets + (bucket, part) -> thread maps for every accumulation level
// grid = batch, block = PLAN_THREADS.   plan layout per MSM: (1 + nlevels) arrays of NBUCKET+1:
//   [0] off   : entry offsets of the sorted list            (off[NBUCKET] = #non-zero digits)
//   [1] tp0   : thread prefix of level 0, parts = max(1, ceil(count / L0))
//   [l] tp(l-1): thread prefix of level l-1 over the previous level's parts
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *lds, uint32_t *total) {
    // wave-level inclusive scan by shuffles, then one wave scans the per-wave totals (<= 16 waves)
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, nwaves = blockDim.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        uint32_t y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    if (wave == 0) {
        uint32_t w = lane < nwaves ? lds[lane] : 0;
#pragma unroll
        for (uint32_t d = 1; d < 64; d <<= 1) {
            uint32_t y = __shfl_up(w, d, 64);
            if (lane >= d) w += y;
        }
        if (lane < nwaves) lds[lane] = w;      // inclusive prefix of wave totals
    }
    __syncthreads();
    uint32_t base = wave ? lds[wave - 1] : 0;
    *total = lds[nwaves - 1];
    __syncthreads();
    return base + x - v;
}

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t *lds) {
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6, nwaves = blockDim.x >> 6;
#pragma unroll
    for (uint32_t d = 32; d >= 1; d >>= 1) {
        uint32_t y = __shfl_xor(v, d, 64);
        v = y > v ? y : v;
    }
    if (lane == 0) lds[wave] = v;
    __syncthreads();
    uint32_t m = 0;
    for (uint32_t w = 0; w < nwaves; ++w) m = lds[w] > m ? lds[w] : m;
    __syncthreads();
    return m;
}

// plan[level] arrays as described above; the last 4 words of the plan hold
//   [0] levels_needed : number of thread-sequential levels (>= 1) before the wavefront-level pass --
//       decided HERE from the actual heaviest bucket, so the common (balanced) case runs level 0 only
//       and later k_accum1 launches exit immediately.
__global__ void SRS_KERNEL_BOUNDS(PLAN_THREADS, 1)
    k_plan(const uint32_t *__restrict__ count, uint32_t *__restrict__ cursor, uint32_t *__restrict__ plan,
           size_t plan_stride, int nlevels, uint32_t l0_log, uint32_t l1_log,
           const uint32_t *__restrict__ seg_off /* wide windows: entry offsets are absolute, segment m starts at seg_off[m] */) {
    // grid = (batch, nlevels + 1): workgroup (m, y) scans ONE array of MSM m -- y = 0 the raw counts (entry offsets), y = l + 1 the
    // part counts of level l -- over all 2^15 buckets.  The arrays only depend on the counts (parts of level l = ceil(parts of level
    // l - 1 / 2^l1_log)), so the levels do not wait for each other (r03: one workgroup did them in turn, 45-55 us of pure latency
    // per MSM launch; now ~one round).  Every workgroup derives the number of levels actually needed the same way.
    // Thread t owns PER consecutive buckets.  r05: they stay in LDS (index i at i + i / PER: conflict-free for the owner's walk AND for the
    // coalesced loads / stores) and are walked -- sum, then running prefix written in place -- instead of being held in 32 registers: the
    // register form spilled 392 bytes per lane to scratch (31 us per launch; k_plan_s, which got this form in r04, takes 14).
    constexpr uint32_t PER = NBUCKET / PLAN_THREADS;             // 32
    __shared__ uint32_t tile[NBUCKET + NBUCKET / PER];
    __shared__ uint32_t lds[64];
    const uint32_t t = threadIdx.x;
    const uint32_t m = blockIdx.x;
    const int my_level = (int)blockIdx.y - 1;
    const uint32_t *cnt = count + (size_t)m * NBUCKET;
    uint32_t *cur = cursor + (size_t)m * NBUCKET;
    uint32_t *pl = plan + (size_t)m * plan_stride;
    {   // all 32 loads of a thread in flight at once (the counters were just written by another XCD's atomics: every load misses this L2)
        uint32_t c[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) c[j] = cnt[t + j * PLAN_THREADS];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t i = t + j * PLAN_THREADS;
            tile[i + i / PER] = c[j];
        }
    }
    __syncthreads();
    const uint32_t base = t * PER + t;
    // parts of a bucket with c entries on level `level` (>= 1: an empty bucket still owns one, identity, part)
    auto value = [&](uint32_t c, int level) -> uint32_t {
        uint32_t p = (c + (1u << l0_log) - 1) >> l0_log;
        p = p ? p : 1u;
        for (int l = 0; l < level; ++l) p = (p + (1u << l1_log) - 1) >> l1_log;
        return p;
    };
    uint32_t local = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < PER; ++j) local += tile[base + j];
    uint32_t total_entries;
    uint32_t run = block_exclusive_scan(local, lds, &total_entries);
    uint32_t total = total_entries;
    int needed = nlevels;
    if (my_level >= 0) {
        // (a) the heaviest bucket must be down to <= FINAL_FANIN parts for the wave-level pass;
        // (b) the TYPICAL bucket (2x the mean load) must be down to one part: the wave-level pass
        //     spends a whole wavefront per bucket, so it must find real work only in outliers.
        uint32_t mx = 0;
#pragma unroll 8
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t v = value(tile[base + j], 0);
            mx = v > mx ? v : mx;
        }
        uint32_t p = block_max(mx, lds);
        needed = 1;
        while (p > FINAL_FANIN && needed < nlevels) {
            p = (p + (1u << l1_log) - 1) >> l1_log;
            ++needed;
        }
        const uint32_t typical = (2u * total_entries + NBUCKET - 1) / NBUCKET;
        uint32_t x = (typical + (1u << l0_log) - 1) >> l0_log;
        int by_mean = 1;
        while (x > 1 && by_mean < nlevels) {
            x = (x + (1u << l1_log) - 1) >> l1_log;
            ++by_mean;
        }
        needed = by_mean > needed ? by_mean : needed;
        if (t == 0 && my_level == 0) pl[plan_stride - 4] = (uint32_t)needed;
        if (my_level >= needed) return;                  // a level nobody runs (workgroup-uniform)
        local = 0;
#pragma unroll 8
        for (uint32_t j = 0; j < PER; ++j) local += value(tile[base + j], my_level);
        run = block_exclusive_scan(local, lds, &total);
    }
    uint32_t mx_own = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < PER; ++j) {
        const uint32_t c = tile[base + j], v = my_level < 0 ? c : value(c, my_level);
        tile[base + j] = run;
        run += v;
        mx_own = v > mx_own ? v : mx_own;
    }
    __syncthreads();
    uint32_t *o = pl + (size_t)(my_level + 1) * (NBUCKET + 1);
    const uint32_t shift = (my_level < 0 && seg_off) ? seg_off[m] : 0u;
    for (uint32_t i = t; i < NBUCKET; i += PLAN_THREADS) {
        const uint32_t v = tile[i + i / PER] + shift;
        o[i] = v;
        if (my_level < 0) cur[i] = v;
    }
    if (t == PLAN_THREADS - 1) o[NBUCKET] = total + shift;
    // every bucket already a single part after the last level?  Then the wave-level pass is a pure copy:
    // k_accum_final exits and k_rowcol reads the last level's parts directly (part index == bucket index).
    if (my_level == needed - 1) {
        const uint32_t p = block_max(mx_own, lds);
        if (t == 0) pl[plan_stride - 3] = (p <= 1u) ? 1u : 0u;
    }
}

// ---- slot mode (msm.h: SLOT_LOG) ---------------------------------------------------------------------------------------------
// k_plan_s: the plan of one set in slot mode.   grid = (batch, nlevels + 2), block = PLAN_THREADS.   Arrays of NBUCKET + 1 per MSM:
//   [0]            off  : entry offsets of the sorted list (as k_plan)
//   [1]            tpo  : prefix of the OVERFLOW parts  max(0, parts(b) - (S - 1))   (level 0 of the overflow levels: these parts start
//                         from the identity and leave a partial sum in `ping`, which k_accum1 / k_ovf_final combine into slot S - 1)
//   [2 .. nlevels]      : prefix of the overflow parts after each further level (ceil(. / 2^l1_log))
//   [nlevels + 1]  tp0  : prefix of ALL level-0 parts  parts(b) = ceil(count(b) / 2^l0)  -- the dense thread space of k_accum0s
// The part length 2^l0 is chosen HERE from the mean bucket load, so that a typical bucket (mean + 6 sigma of a Poisson load) fits its
// S - 1 regular slots whatever the share of zero digits, and small sets get short parts (more threads): every workgroup derives the
// same value.  Header (last 4 words): [0] overflow levels needed, [1] 0, [2] l0, [3] overflow parts (also written to *h_ovf, which
// the host reads after the stream has been synchronised: msm::overflow_missed).
__device__ __forceinline__ uint32_t slot_l0_log(uint32_t total_entries, uint32_t S, uint32_t want_cap) {
    const uint32_t mean = total_entries / NBUCKET;
    uint32_t r = 0;
    while ((r + 1) * (r + 1) <= mean) ++r;                       // isqrt: <= 256 rounds, workgroup-uniform
    const uint32_t thresh = mean + 6 * r + 1;
    uint32_t lg = SLOT_L0_MIN_LOG;
    while (((thresh + (1u << lg) - 1) >> lg) > S - 1 && lg < SLOT_L0_MAX_LOG) ++lg;
    // not shorter than needed to fill the chip ~2.5 times over (2^19 threads), up to the 16 entries that amortise a part's load / store
    uint32_t want = 0;
    while (want < want_cap && (total_entries >> (19 + want + 1)) != 0) ++want;
    return lg > want ? lg : want;
}

__global__ void SRS_KERNEL_BOUNDS(PLAN_THREADS, 1)
    k_plan_s(const uint32_t *__restrict__ count, uint32_t *__restrict__ cursor, uint32_t *__restrict__ plan, size_t plan_stride, int nlevels,
             uint32_t S, uint32_t l1_log, const uint8_t *__restrict__ used_prev, uint8_t *__restrict__ used_next, int first,
             uint32_t *__restrict__ h_ovf, uint32_t want_cap) {
    // Thread t owns PER consecutive buckets; they stay in LDS (index i at i + i / PER: conflict-free for the owner's walk AND for the
    // coalesced loads / stores) and are walked twice -- sum, then running prefix written in place -- instead of being held in 32 registers
    // (k_plan's form spilled 100+ bytes per lane to scratch: 34 us per launch, a third of a small chunk's fixed cost).
    constexpr uint32_t PER = NBUCKET / PLAN_THREADS;             // 32
    __shared__ uint32_t tile[NBUCKET + NBUCKET / PER];
    __shared__ uint32_t lds[64];
    const uint32_t t = threadIdx.x, m = blockIdx.x, role = blockIdx.y;
    const uint32_t *cnt = count + (size_t)m * NBUCKET;
    uint32_t *pl = plan + (size_t)m * plan_stride;
    {   // all 32 loads of a thread in flight at once: issued one per loop round they cost a memory latency EACH (the counters were just
        // written by another XCD's atomics: every load misses this XCD's L2) -- that, not arithmetic, was the 30+ us of this kernel
        uint32_t c[PER];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) c[j] = cnt[t + j * PLAN_THREADS];
#pragma unroll
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t i = t + j * PLAN_THREADS;
            tile[i + i / PER] = c[j];
        }
    }
    __syncthreads();
    const uint32_t base = t * PER + t;
    uint32_t local = 0;
#pragma unroll 8
    for (uint32_t j = 0; j < PER; ++j) local += tile[base + j];
    uint32_t total_entries;
    uint32_t run = block_exclusive_scan(local, lds, &total_entries);
    const uint32_t l0_log = slot_l0_log(total_entries, S, want_cap);
    uint32_t total = total_entries;
    const bool dense = role == (uint32_t)nlevels + 1;
    const uint32_t lv = role >= 2 && !dense ? role - 1 : 0;      // further levels an overflow role applies
    // the value of a bucket with c entries in this role's array
    auto value = [&](uint32_t c) -> uint32_t {
        if (role == 0) return c;
        uint32_t p = (c + (1u << l0_log) - 1) >> l0_log;         // level-0 parts
        if (dense) return p;
        p = p > S - 1 ? p - (S - 1) : 0u;                        // ... beyond the regular slots
        for (uint32_t l = 0; l < lv; ++l) p = (p + (1u << l1_log) - 1) >> l1_log;
        return p;
    };
    if (role != 0) {
        local = 0;
        uint32_t mx = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < PER; ++j) {
            const uint32_t c = tile[base + j];
            local += value(c);
            if (!dense) {
                const uint32_t p = (c + (1u << l0_log) - 1) >> l0_log, o = p > S - 1 ? p - (S - 1) : 0u;
                mx = o > mx ? o : mx;
            }
        }
        if (!dense) {
            uint32_t p = block_max(mx, lds);
            int needed = 1;
            while (p > FINAL_FANIN && needed < nlevels) {
                p = (p + (1u << l1_log) - 1) >> l1_log;
                ++needed;
            }
            if (role == 1 && t == 0) {
                pl[plan_stride - 4] = (uint32_t)needed;
                pl[plan_stride - 3] = 0;
                pl[plan_stride - 2] = l0_log;
            }
            if ((int)role - 1 >= needed) return;                 // a level nobody runs (workgroup-uniform)
        }
        run = block_exclusive_scan(local, lds, &total);
    }
    // slots in use after this set: the thread's 32 bytes travel as two 16-byte words (byte loads in the loop cost a memory latency EACH:
    // that was 25 of this kernel's 33 us)
    static_assert(PER == 32, "k_plan_s: used[] travels as 2 x uint4 per thread");
    uint32_t was_w[8] = {0, 0, 0, 0, 0, 0, 0, 0}, now_w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (dense && !first) {
        const uint4 *up = reinterpret_cast<const uint4 *>(used_prev + (size_t)m * NBUCKET + (size_t)t * PER);
        const uint4 a = up[0], b = up[1];
        was_w[0] = a.x; was_w[1] = a.y; was_w[2] = a.z; was_w[3] = a.w; was_w[4] = b.x; was_w[5] = b.y; was_w[6] = b.z; was_w[7] = b.w;
    }
#pragma unroll
    for (uint32_t j = 0; j < PER; ++j) {
        const uint32_t c = tile[base + j], v = value(c);
        tile[base + j] = run;
        run += v;
        if (dense) {
            const uint32_t now = v < S - 1 ? v : S - 1, was = (was_w[j >> 2] >> (8 * (j & 3))) & 0xFFu;
            now_w[j >> 2] |= (now > was ? now : was) << (8 * (j & 3));
        }
    }
    if (dense) {
        uint4 *un = reinterpret_cast<uint4 *>(used_next + (size_t)m * NBUCKET + (size_t)t * PER);
        uint4 lo, hi;
        lo.x = now_w[0]; lo.y = now_w[1]; lo.z = now_w[2]; lo.w = now_w[3];
        hi.x = now_w[4]; hi.y = now_w[5]; hi.z = now_w[6]; hi.w = now_w[7];
        un[0] = lo;
        un[1] = hi;
    }
    __syncthreads();
    uint32_t *o = pl + (size_t)role * (NBUCKET + 1);
    uint32_t *cur = cursor + (size_t)m * NBUCKET;
    for (uint32_t i = t; i < NBUCKET; i += PLAN_THREADS) {
        const uint32_t v = tile[i + i / PER];
        o[i] = v;
        if (role == 0) cur[i] = v;
    }
    if (t == PLAN_THREADS - 1) {
        o[NBUCKET] = total;
        if (role == 1) {
            pl[plan_stride - 1] = total;
            h_ovf[m] = total;
        }
        if (role == 0) h_ovf[(size_t)LANDING_SLOTS * BATCH_ARGS + m] = total;      // the set's non-zero digits (msm::note_commit: the witness's density)
    }
}

// `nseg`: the segments that k_plan ran for; the others (a plain key of form 2 populates 8 of the 16) own no part on any level, so that
// base[l][nseg .. NSEG_W] all hold the number of parts and link_segment never names one of them
// NS > 64 (the batched plain flow): one thread per segment of capacity, block = NS, the scan goes through LDS.
template <uint32_t NS = NSEG_W>
__global__ void k_link(const uint32_t *__restrict__ plan, size_t plan_stride, int nlevels, LinkT<NS> *__restrict__ link, uint32_t nseg) {
    const uint32_t t = threadIdx.x;
    if constexpr (NS > 64) {
        __shared__ uint32_t lds[64];
        for (int l = 0; l < nlevels; ++l) {                       // workgroup-uniform
            uint32_t c = 0;
            if (t < nseg) {
                const uint32_t *pl = plan + (size_t)t * plan_stride;
                if ((uint32_t)l < pl[plan_stride - 4]) c = pl[(size_t)(l + 1) * (NBUCKET + 1) + NBUCKET];
            }
            uint32_t total;
            const uint32_t ex = block_exclusive_scan(c, lds, &total);
            if (t < NS) link->base[l][t] = ex;
            if (t == 0) link->base[l][NS] = total;
        }
        return;
    }
    for (int l = 0; l < nlevels; ++l) {
        uint32_t c = 0;
        if (t < nseg) {
            const uint32_t *pl = plan + (size_t)t * plan_stride;
            if ((uint32_t)l < pl[plan_stride - 4]) c = pl[(size_t)(l + 1) * (NBUCKET + 1) + NBUCKET];
        }
        uint32_t x = c;
#pragma unroll
        for (uint32_t d = 1; d < NSEG_W; d <<= 1) {
            uint32_t y = __shfl_up(x, d, 64);
            if (t >= d) x += y;
        }
        if (t < NSEG_W) link->base[l][t] = x - c;
        if (t == NSEG_W - 1) link->base[l][NSEG_W] = x;
    }
}

// ---------------------------------------------------------------------------------------------
// 4. bucket accumulation
// level 0: thread t = (bucket, part): <= L0 gathered mixed adds  ->  parts0[t]  (XYZZ)
// grid = (blocks, batch)
// ---------------------------------------------------------------------------------------------
// thread -> bucket map of level 0: tb[t] = b for tp0[b] <= t < tp0[b + 1].  k_accum0 used to find its bucket by a binary search
// over the 2^15 prefix entries -- 15 DEPENDENT global loads (~15 us) in front of ~130 us of additions, in every thread.
// One wavefront per bucket writes the (contiguous) range instead; the map is 2 bytes per thread.   grid = (NBUCKET / 4, batch)
template <uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(256, 1)
    k_expand(const uint32_t *__restrict__ plan, size_t plan_stride, uint16_t *__restrict__ tb, size_t tb_stride,
             const LinkT<NS> *__restrict__ link, uint32_t arr /* plan array holding the thread prefix: 1, or nlevels + 1 in slot mode */) {
    const uint32_t m = blockIdx.y, lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint32_t *tp = plan + (size_t)m * plan_stride + (size_t)arr * (NBUCKET + 1);
    uint16_t *out = tb + (link ? (size_t)link->base[0][m] : (size_t)m * tb_stride);
    const uint32_t s = tp[b], e = tp[b + 1];
    for (uint32_t t = s + lane; t < e; t += 64) out[t] = (uint16_t)b;
}

// The chain of gathered mixed additions of one level-0 part: init (nullptr: the identity) + sum of the entries src[s .. e), s < e.
// Behind every addition travel the NEXT gathered point (its index arrived an addition ago) and the index after it (r04: with the index
// loaded in the same round as the gather it addresses, every round parked the wave for a memory latency).
// r06: the loop runs the addition WITHOUT its exceptional cases (Ec29::madd_signed_fast: no identity tests, no branch, no doubling
// path in the loop body); a chain that met one -- an identity entry of a degenerate key, a partial sum that cancelled, an entry equal to
// the running sum -- is detected by a sticky flag and recomputed from its start with the complete formulas.
// COMPACT (compact keys, msm.h): bit 30 of an entry says that its point is phi(T[index]) = (beta x, y): the gathered x is multiplied by
// beta.  The product does not depend on the running sum, so it sits beside the chain.  It is a per-lane BRANCH; the alternative, an
// unconditional product with beta-or-one, measured within 3 % either way on a resident 2^24 MSM (uniform scalars: branch 22.4 ms, select
// 22.6; 55 % zeros: branch 11.2-11.3, select 10.95; profiles/compact_key_ab.txt) -- the branch keeps 130 / 131 VGPRs against 134 / 129 and
// lets a wavefront whose parts hold no flagged entry (scalars below 2^64 have k2 = 0) skip the product.
// A table identity (0, 0) stays (0, 0) exactly -- the product of 0 is 0 --, so the exceptional-case tests of the chain hold unchanged.
template <class C, bool COMPACT>
__device__ __forceinline__ aff29_t load_entry(const affine_t &p, uint32_t v) {
    aff29_t q = Ec29<C>::load_raw(p);
    if (COMPACT) {
        if (v & PAY_ENDO) {
            f29_t beta;
#pragma unroll
            for (int i = 0; i < 9; ++i) beta.v[i] = GlvConsts<C::ID>::beta29(i);
            q.x = Ec29<C>::F::mul(q.x, beta);        // < 2P norm: within the bounds of every use of a table x (curve29.cuh)
        }
    }
    return q;
}
template <bool COMPACT>
__device__ __forceinline__ uint32_t entry_index(uint32_t v) { return v & (COMPACT ? PAY_ENDO - 1u : 0x7FFFFFFFu); }

template <class C, bool COMPACT>
__device__ __forceinline__ xyzz29_t accumulate_part(const uint32_t *__restrict__ src, uint32_t s, uint32_t e, const affine_t *__restrict__ table,
                                                    const xyzz_t *__restrict__ init) {
    using E29 = Ec29<C>;
    using F = typename E29::F;
    bool exc = false;
    xyzz29_t acc;
    {
        uint32_t v = src[s];
        uint32_t vn = s + 1 < e ? src[s + 1] : 0u;
        affine_t p = table[entry_index<COMPACT>(v)];
        uint32_t j = s;
        if (init) {
            acc = E29::unpack(*init);
        } else {                              // a fresh part: the first entry IS the sum so far
            affine_t pn = p;
            uint32_t vnn = 0;
            if (s + 1 < e) {
                pn = table[entry_index<COMPACT>(vn)];
                if (s + 2 < e) vnn = src[s + 2];
            }
            const aff29_t q = load_entry<C, COMPACT>(p, v);
            acc.x = q.x;
            acc.y = (v >> 31) ? F::normalize(F::template neg_lazy<1, 0>(q.y)) : q.y;      // P - y  (y != 0 unless Q = O: flagged)
            acc.zz = E29::one();
            acc.zzz = acc.zz;
            exc = F::is_zero_exact(q.y);
            v = vn;
            vn = vnn;
            p = pn;
            j = s + 1;
        }
        for (; j < e; ++j) {
            uint32_t vnn = 0;
            affine_t pn = p;
            if (j + 1 < e) {
                pn = table[entry_index<COMPACT>(vn)];
                if (j + 2 < e) vnn = src[j + 2];
            }
            acc = E29::madd_signed_fast(acc, load_entry<C, COMPACT>(p, v), (v >> 31) != 0, exc);
            v = vn;
            vn = vnn;
            p = pn;
        }
    }
    if (exc) {                                // rare: once more, complete
        acc = init ? E29::unpack(*init) : E29::identity();
#pragma unroll 1
        for (uint32_t j = s; j < e; ++j) {
            const uint32_t v = src[j];
            acc = E29::madd_signed(acc, load_entry<C, COMPACT>(table[entry_index<COMPACT>(v)], v), (v >> 31) != 0);
        }
    }
    return acc;
}

template <class C, bool COMPACT, uint32_t NS = NSEG_W>
__device__ __forceinline__ void accum0_thread(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan,
                                              size_t plan_stride, const uint16_t *__restrict__ tb, size_t tb_stride,
                                              const affine_t *__restrict__ table, xyzz_t *__restrict__ parts, size_t parts_stride, uint32_t l0,
                                              const LinkT<NS> *__restrict__ link) {
    uint32_t m = blockIdx.y;
    uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    size_t slot;                                   // index of this thread's part (and map entry)
    if (link) {                                    // wide windows: flat thread space over the segments, offsets are absolute
        if (t >= link->base[0][NS]) return;
        m = link_segment<NS>(link->base[0], t);
        slot = t;
        t -= link->base[0][m];
    } else {
        slot = (size_t)m * parts_stride + t;
    }
    const uint32_t *off = plan + (size_t)m * plan_stride;
    const uint32_t *tp = off + (NBUCKET + 1);
    if (t >= tp[NBUCKET]) return;
    uint32_t b = tb[link ? slot : (size_t)m * tb_stride + t];
    uint32_t part = t - tp[b];
    uint32_t s = off[b] + part * l0;
    uint32_t e = off[b + 1];
    if (e > s + l0) e = s + l0;
    const uint32_t *src = link ? sorted : sorted + (size_t)m * sorted_stride;
    // the additions run on the 9 x 29-bit limb form (curve29.cuh); the table is stored in its Montgomery form
    using E29 = Ec29<C>;
    const xyzz29_t acc = s < e ? accumulate_part<C, COMPACT>(src, s, e, table, nullptr) : E29::identity();
    parts[slot] = E29::pack(acc);                                // canonical R'-form: the later levels stay on the 29-bit multiplier
}
template <class C, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(ACC_THREADS, 1)
    k_accum0(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan,
             size_t plan_stride, const uint16_t *__restrict__ tb, size_t tb_stride, const affine_t *__restrict__ table,
             xyzz_t *__restrict__ parts, size_t parts_stride, uint32_t l0, const LinkT<NS> *__restrict__ link) {
    accum0_thread<C, false, NS>(sorted, sorted_stride, plan, plan_stride, tb, tb_stride, table, parts, parts_stride, l0, link);
}
// the same for a compact key (entries flagged PAY_ENDO): a kernel of its own, so that the one full keys launch is compiled as before
template <class C, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(ACC_THREADS, 1)
    k_accum0c(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan,
              size_t plan_stride, const uint16_t *__restrict__ tb, size_t tb_stride, const affine_t *__restrict__ table,
              xyzz_t *__restrict__ parts, size_t parts_stride, uint32_t l0, const LinkT<NS> *__restrict__ link) {
    accum0_thread<C, true, NS>(sorted, sorted_stride, plan, plan_stride, tb, tb_stride, table, parts, parts_stride, l0, link);
}

// 64-lane exchange of an XYZZ point
__device__ __forceinline__ xyzz_t shfl_down_point(const xyzz_t &p, unsigned delta) {
    xyzz_t o;
    shfl_down_words<32>(reinterpret_cast<const uint32_t *>(&p), reinterpret_cast<uint32_t *>(&o), delta, 64);
    return o;
}

// 64-lane exchange of a point in 9-limb coordinates (36 words), inside groups of `width` lanes
__device__ __forceinline__ xyzz29_t shfl_down_point29(const xyzz29_t &p, unsigned delta, int width) {
    xyzz29_t o;
    shfl_down_words<36>(reinterpret_cast<const uint32_t *>(&p), reinterpret_cast<uint32_t *>(&o), delta, width);
    return o;
}

// level >= 1: (bucket, part) over the previous level's parts, <= L1 full adds each.
// Two modes, chosen on the device from the number of outputs of this level:
//   many outputs  -> one lane per output (throughput-bound, every lane runs its own additions)
//   few outputs   -> one QUAD per output (latency-bound tail: Ec::add_quad cuts the dependent chain 3.3x)
// The grid is sized for the quad mode; in lane mode the surplus workgroups exit.
template <class C, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(ACC_THREADS, 1)
    k_accum1(const xyzz_t *__restrict__ in, size_t in_stride, const uint32_t *__restrict__ plan,
             size_t plan_stride, int level, xyzz_t *__restrict__ out, size_t out_stride, uint32_t l1,
             const LinkT<NS> *__restrict__ link, uint32_t quad_max) {
    uint32_t m = blockIdx.y;
    const uint32_t lin = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t t;
    bool quad;
    size_t in_off, out_off;
    if (link) {                                // wide windows: flat thread space of this level over the segments
        const uint32_t n_all = link->base[level][NS];
        quad = n_all <= quad_max;
        t = quad ? (lin >> 2) : lin;
        if (t >= n_all) return;
        m = link_segment<NS>(link->base[level], t);
        t -= link->base[level][m];
        in_off = link->base[(level - 1) & 1][m];
        out_off = link->base[level & 1][m];
    } else {
        in_off = (size_t)m * in_stride;
        out_off = (size_t)m * out_stride;
    }
    if ((uint32_t)level >= plan[(size_t)m * plan_stride + plan_stride - 4]) return;   // level not needed (k_plan)
    const uint32_t *tp_prev = plan + (size_t)m * plan_stride + (size_t)level * (NBUCKET + 1);
    const uint32_t *tp = tp_prev + (NBUCKET + 1);
    const uint32_t n_out = tp[NBUCKET];
    if (!link) {
        quad = (uint64_t)n_out * gridDim.y <= quad_max;   // whole batch: latency-bound only while the chip is not full
        t = quad ? (lin >> 2) : lin;
    }
    if (t >= n_out) return;                    // in quad mode the 4 lanes of a quad leave together
    uint32_t b = upper_bucket(tp, t);
    uint32_t part = t - tp[b];
    uint32_t s = tp_prev[b] + part * l1;
    uint32_t e = tp_prev[b + 1];
    if (e > s + l1) e = s + l1;
    using E29 = Ec29<C>;
    const xyzz_t *src = in + in_off;
    xyzz29_t acc = E29::unpack(src[s]);
    if (quad) {
        const uint32_t q = threadIdx.x & 3u;
        for (uint32_t j = s + 1; j < e; ++j) acc = E29::add_quad(acc, E29::unpack(src[j]), q);
        if (q == 0) out[out_off + t] = E29::pack(acc);
    } else {
        for (uint32_t j = s + 1; j < e; ++j) acc = E29::add(acc, E29::unpack(src[j]));
        out[out_off + t] = E29::pack(acc);
    }
}

// final level: one wavefront per bucket; lanes stride over the remaining parts, then a 6-step
// shuffle tree; lane 0 stores the bucket.   grid = (NBUCKET / waves_per_block, batch)
template <class C, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(FINAL_THREADS, 1)
    k_accum_final(const xyzz_t *__restrict__ ping, size_t ping_stride, const xyzz_t *__restrict__ pong,
                  size_t pong_stride, const uint32_t *__restrict__ plan, size_t plan_stride,
                  xyzz_t *__restrict__ buckets, const LinkT<NS> *__restrict__ link) {
    uint32_t m = blockIdx.y;
    if (plan[(size_t)m * plan_stride + plan_stride - 3]) return;              // all buckets single: nothing to combine
    const uint32_t level = plan[(size_t)m * plan_stride + plan_stride - 4];   // levels actually run
    const xyzz_t *in = (level & 1u) ? ping : pong;     // level 0 -> ping, level 1 -> pong, ...
    const size_t in_stride = (level & 1u) ? ping_stride : pong_stride;
    const uint32_t *tp = plan + (size_t)m * plan_stride + (size_t)level * (NBUCKET + 1);
    uint32_t lane = threadIdx.x & 63u;
    uint32_t b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    uint32_t s = tp[b], e = tp[b + 1];
    const xyzz_t *src = in + (link ? (size_t)link->base[(level - 1u) & 1u][m] : (size_t)m * in_stride);
    xyzz_t *dst = buckets + (size_t)m * NBUCKET;
    if (e - s == 1) {                       // common case: the bucket is already one part
        if (lane == 0) dst[b] = src[s];
        return;
    }
    using E29 = Ec29<C>;
    xyzz29_t acc = E29::identity();
    for (uint32_t j = s + lane; j < e; j += 64) acc = E29::add(acc, E29::unpack(src[j]));
    for (unsigned d = 32; d >= 1; d >>= 1) {
        xyzz29_t other = shfl_down_point29(acc, d, 64);
        if (lane < d) acc = E29::add(acc, other);
    }
    if (lane == 0) dst[b] = E29::pack(acc);
}

// ---- slot mode: bucket accumulation INTO the persistent slots ------------------------------------------------------------------
// thread t = (bucket b, part p) of the dense thread space tp0 (plan array `arr`): <= 2^l0 gathered mixed additions, like k_accum0, but
//   p <  S - 1 : the running sum of slot (b, p) is the start value (identity when the slot holds nothing yet) and the result goes back
//                -- nothing is left for later levels to combine, whatever the number of sets a commit is cut into;
//   p >= S - 1 : a hot bucket (more entries than S - 1 parts hold): a fresh partial sum into `ovf`, combined by k_accum1 / k_ovf_final.
// grid = (ceil(cap / ACC_THREADS), batch)
template <class C, bool COMPACT>
__device__ __forceinline__ void accum0s_thread(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan,
                                               size_t plan_stride, uint32_t arr, const uint16_t *__restrict__ tb, size_t tb_stride,
                                               const affine_t *__restrict__ table, xyzz_t *__restrict__ slots, uint32_t S,
                                               const uint8_t *__restrict__ used_prev, int first, xyzz_t *__restrict__ ovf, size_t ovf_stride) {
    const uint32_t m = blockIdx.y;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t *off = plan + (size_t)m * plan_stride;
    const uint32_t *tp = off + (size_t)arr * (NBUCKET + 1);
    if (t >= tp[NBUCKET]) return;
    const uint32_t *tpo = off + (NBUCKET + 1);
    const uint32_t l0 = 1u << off[plan_stride - 2];
    const uint32_t b = tb[(size_t)m * tb_stride + t];
    const uint32_t part = t - tp[b];
    uint32_t s = off[b] + part * l0;
    uint32_t e = off[b + 1];
    if (e > s + l0) e = s + l0;
    const uint32_t *src = sorted + (size_t)m * sorted_stride;
    using E29 = Ec29<C>;
    const bool regular = part < S - 1;
    xyzz_t *slot = regular ? slots + ((size_t)m * NBUCKET + b) * S + part : ovf + (size_t)m * ovf_stride + tpo[b] + (part - (S - 1));
    // a part is never empty (s < e); the slot's running sum is the start value when the slot holds one
    const bool resume = regular && !first && part < (uint32_t)used_prev[(size_t)m * NBUCKET + b];
    *slot = E29::pack(accumulate_part<C, COMPACT>(src, s, e, table, resume ? slot : nullptr));
}
template <class C>
__global__ void SRS_KERNEL_BOUNDS(ACC_THREADS, 1)
    k_accum0s(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan, size_t plan_stride, uint32_t arr,
              const uint16_t *__restrict__ tb, size_t tb_stride, const affine_t *__restrict__ table, xyzz_t *__restrict__ slots, uint32_t S,
              const uint8_t *__restrict__ used_prev, int first, xyzz_t *__restrict__ ovf, size_t ovf_stride) {
    accum0s_thread<C, false>(sorted, sorted_stride, plan, plan_stride, arr, tb, tb_stride, table, slots, S, used_prev, first, ovf, ovf_stride);
}
template <class C>
__global__ void SRS_KERNEL_BOUNDS(ACC_THREADS, 1)
    k_accum0sc(const uint32_t *__restrict__ sorted, size_t sorted_stride, const uint32_t *__restrict__ plan, size_t plan_stride, uint32_t arr,
               const uint16_t *__restrict__ tb, size_t tb_stride, const affine_t *__restrict__ table, xyzz_t *__restrict__ slots, uint32_t S,
               const uint8_t *__restrict__ used_prev, int first, xyzz_t *__restrict__ ovf, size_t ovf_stride) {
    accum0s_thread<C, true>(sorted, sorted_stride, plan, plan_stride, arr, tb, tb_stride, table, slots, S, used_prev, first, ovf, ovf_stride);
}

// the wave-level pass of the overflow parts: one wavefront per bucket sums what the overflow levels left of it and adds the sum into the
// bucket's LAST slot (first set of a commit: every bucket's last slot is initialised here).   grid = (NBUCKET / waves_per_block, batch)
template <class C>
__global__ void SRS_KERNEL_BOUNDS(FINAL_THREADS, 1)
    k_ovf_final(const xyzz_t *__restrict__ ping, size_t ping_stride, const xyzz_t *__restrict__ pong, size_t pong_stride,
                const uint32_t *__restrict__ plan, size_t plan_stride, xyzz_t *__restrict__ slots, uint32_t S, int first) {
    const uint32_t m = blockIdx.y;
    const uint32_t level = plan[(size_t)m * plan_stride + plan_stride - 4];   // overflow levels actually run
    const xyzz_t *in = (level & 1u) ? ping + (size_t)m * ping_stride : pong + (size_t)m * pong_stride;     // level 0 -> ping, level 1 -> pong, ...
    const uint32_t *tp = plan + (size_t)m * plan_stride + (size_t)level * (NBUCKET + 1);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint32_t s = tp[b], e = tp[b + 1];
    xyzz_t *dst = slots + ((size_t)m * NBUCKET + b) * S + (S - 1);
    using E29 = Ec29<C>;
    if (e == s) {                            // the usual bucket: nothing beyond its regular slots
        if (first && lane == 0) *dst = E29::pack(E29::identity());
        return;
    }
    xyzz29_t acc = E29::identity();
    for (uint32_t j = s + lane; j < e; j += 64) acc = E29::add(acc, E29::unpack(in[j]));
    for (unsigned d = 32; d >= 1; d >>= 1) {
        xyzz29_t other = shfl_down_point29(acc, d, 64);
        if (lane < d) acc = E29::add(acc, other);
    }
    if (lane == 0) {
        if (!first) acc = E29::add(acc, E29::unpack(*dst));
        *dst = E29::pack(acc);
    }
}

// the reduction of the slots at the end of a commit, <= 8 inputs per output: out[B * out_pb + g] = sum_j in[B * in_pb + g + j * out_pb] over
// the inputs that hold a sum -- index < used[B] (first level; nullptr: all of them) or == extra (the overflow slot, when its kernels ran).
// B = m * NBUCKET + b.  The inputs of an output are STRIDED (a bucket with u slots in use gives every one of its outputs u / out_pb of
// them, whatever u) and the thread space is g-major (a wavefront = 64 buckets at the same g: the wavefronts of a level carry equal
// chains, and a small MSM with one or two slots per bucket in use runs a few full wavefronts instead of one lane in eight of all of them).
// QUAD: one quad per output (the last level: 2^15 outputs per MSM).   grid = (ceil(n_out [* 4] / 256), batch)
template <class C, bool QUAD>
__global__ void SRS_KERNEL_BOUNDS(256, 1)
    k_slot_reduce(const xyzz_t *__restrict__ in, uint32_t in_pb, const uint8_t *__restrict__ used, size_t used_stride, int extra,
                  xyzz_t *__restrict__ out, uint32_t out_pb) {
    using E29 = Ec29<C>;
    const uint32_t m = blockIdx.y;
    const uint32_t lin = blockIdx.x * blockDim.x + threadIdx.x, t = QUAD ? (lin >> 2) : lin, q = lin & 3u;
    if (t >= NBUCKET * out_pb) return;
    const uint32_t g = t / NBUCKET, b = t % NBUCKET;
    const uint32_t lim = used ? (uint32_t)used[(size_t)m * used_stride + b] : in_pb;
    const xyzz_t *src = in + ((size_t)m * NBUCKET + b) * in_pb;
    xyzz29_t acc = E29::identity();
    for (uint32_t idx = g; idx < in_pb; idx += out_pb) {
        if (!(idx < lim || (int)idx == extra)) continue;                          // uniform inside a quad
        const xyzz29_t x = E29::unpack(src[idx]);
        if (QUAD) acc = E29::add_quad(acc, x, q); else acc = E29::add(acc, x);
    }
    if (!QUAD || q == 0) out[((size_t)m * NBUCKET + b) * out_pb + g] = E29::pack(acc);
}

// chunked commits: the finished buckets of this set (where k_rowcol would read them) go into the key's running buckets;
// one thread per bucket.   grid = NBUCKET / 64
template <class C>
__global__ void SRS_KERNEL_BOUNDS(64, 1)
    k_bucket_fold(const xyzz_t *__restrict__ buckets, const xyzz_t *__restrict__ ping, const xyzz_t *__restrict__ pong,
                  const uint32_t *__restrict__ plan, size_t plan_stride, xyzz_t *__restrict__ total, int first) {
    using E29 = Ec29<C>;
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t *hdr = plan + plan_stride - 4;                              // [0] levels run, [1] all buckets single
    const xyzz_t *B = hdr[1] ? ((hdr[0] & 1u) ? ping : pong) : buckets;
    if (first) {
        total[b] = B[b];
    } else {
        total[b] = E29::pack(E29::add(E29::unpack(total[b]), E29::unpack(B[b])));
    }
}

// the same for the linked segments of the plain flow (one segment = one window of a plain key): segment m's finished buckets, exactly where
// k_rowcol finds them with from_buckets == 0 -- buckets + m NBUCKET when the wave-level pass wrote them, ping / pong at the segment's LINKED
// offset when its plan header says every bucket was single (every small chunk) -- go into total[m][NBUCKET].
// grid = (NBUCKET / 64, segments)
template <class C>
__global__ void SRS_KERNEL_BOUNDS(64, 1)
    k_bucket_fold_seg(const xyzz_t *__restrict__ buckets, const xyzz_t *__restrict__ ping, const xyzz_t *__restrict__ pong,
                      const uint32_t *__restrict__ plan, size_t plan_stride, const Link *__restrict__ link, xyzz_t *__restrict__ total,
                      int first) {
    using E29 = Ec29<C>;
    const uint32_t m = blockIdx.y, b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t *hdr = plan + (size_t)m * plan_stride + plan_stride - 4;   // [0] levels run, [1] all buckets single
    const xyzz_t *B = hdr[1] ? ((hdr[0] & 1u) ? ping + (size_t)link->base[0][m] : pong + (size_t)link->base[1][m])
                             : buckets + (size_t)m * NBUCKET;
    xyzz_t *T = total + (size_t)m * NBUCKET;
    if (first) {
        T[b] = B[b];
    } else {
        T[b] = E29::pack(E29::add(E29::unpack(T[b]), E29::unpack(B[b])));
    }
}

// ---------------------------------------------------------------------------------------------
// 5. bucket reduction  S = sum_b (b+1) B_b,  b = hi * RED_COLS + lo
//    S = RED_COLS * sum_hi hi * R_hi  +  sum_lo (lo+1) * C_lo
// k_rowcol: block < RED_ROWS -> row sum R_hi ; else column sum C_lo.   grid = (ROWS + COLS, batch)
// ---------------------------------------------------------------------------------------------
template <class C>
__device__ __forceinline__ void lds_tree_sum(xyzz_t *v, uint32_t n_pow2) {
    for (uint32_t s = n_pow2 >> 1; s >= 1; s >>= 1) {
        if (threadIdx.x < s) v[threadIdx.x] = Ec<C>::add(v[threadIdx.x], v[threadIdx.x + s]);
        __syncthreads();
    }
}

// 64-lane exchange of an XYZZ point inside groups of `width` lanes
__device__ __forceinline__ xyzz_t shfl_down_point_w(const xyzz_t &p, unsigned delta, int width) {
    xyzz_t o;
    shfl_down_words<32>(reinterpret_cast<const uint32_t *>(&p), reinterpret_cast<uint32_t *>(&o), delta, width);
    return o;
}

// Row / column sums, one QUAD per lane-task (Ec::add_quad): a quad first adds RC_SER consecutive elements, then the
// 16 quads of a wavefront combine by a shuffle tree (partner quad = 4 d lanes further).  A row (128 elements) is one
// wavefront; a column (256 elements) is the two wavefronts of a workgroup, joined through LDS.
// grid = (RED_ROWS / 2 + RED_COLS, batch), block = 128: workgroups < RED_ROWS / 2 do two rows, the others one column.
template <class C, uint32_t NS = NSEG_W>
__global__ void SRS_KERNEL_BOUNDS(128, 1)
    k_rowcol(const xyzz_t *__restrict__ buckets, const xyzz_t *__restrict__ ping, size_t ping_stride,
             const xyzz_t *__restrict__ pong, size_t pong_stride, const uint32_t *__restrict__ plan, size_t plan_stride,
             xyzz_t *__restrict__ rc /* [batch][ROWS + COLS] */, const LinkT<NS> *__restrict__ link, int from_buckets) {
    constexpr uint32_t SER = 8;
    __shared__ xyzz_t half[1];
    const uint32_t m = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t q = lane & 3u, vl = lane >> 2;                                // quad role, quad index 0..15
    const uint32_t *hdr = plan + (size_t)m * plan_stride + plan_stride - 4;   // [0] levels run, [1] all buckets single
    const size_t ping_off = link ? (size_t)link->base[0][m] : (size_t)m * ping_stride;
    const size_t pong_off = link ? (size_t)link->base[1][m] : (size_t)m * pong_stride;
    const xyzz_t *B = (hdr[1] && !from_buckets) ? ((hdr[0] & 1u) ? ping + ping_off : pong + pong_off) : buckets + (size_t)m * NBUCKET;
    using E29 = Ec29<C>;
    xyzz_t *out = rc + (size_t)m * (RED_ROWS + RED_COLS);
    const bool is_row = blockIdx.x < RED_ROWS / 2;
    xyzz29_t acc;
    if (is_row) {
        const uint32_t hi = blockIdx.x * 2 + wave;                               // 16 quads x 8 = 128 = RED_COLS
        const xyzz_t *src = B + (size_t)hi * RED_COLS + vl * SER;
        acc = E29::unpack(src[0]);
        xyzz_t nx = src[1];
        for (uint32_t j = 1; j < SER; ++j) {             // next element is fetched behind the addition
            xyzz_t cur = nx;
            if (j + 1 < SER) nx = src[j + 1];
            acc = E29::add_quad(acc, E29::unpack(cur), q);
        }
    } else {
        const uint32_t lo = blockIdx.x - RED_ROWS / 2, sub = wave * 16 + vl;     // 32 quads x 8 = 256 = RED_ROWS
        const xyzz_t *src = B + (size_t)(sub * SER) * RED_COLS + lo;
        acc = E29::unpack(src[0]);
        xyzz_t nx = src[RED_COLS];
        for (uint32_t j = 1; j < SER; ++j) {
            xyzz_t cur = nx;
            if (j + 1 < SER) nx = src[(size_t)(j + 1) * RED_COLS];
            acc = E29::add_quad(acc, E29::unpack(cur), q);
        }
    }
    for (unsigned d = 8; d >= 1; d >>= 1) {
        xyzz29_t o = shfl_down_point29(acc, 4 * d, 64);
        if (vl < d) acc = E29::add_quad(acc, o, q);
    }
    if (is_row) {
        if (lane == 0) out[blockIdx.x * 2 + wave] = E29::pack(acc);
        return;
    }
    if (wave == 1 && lane == 0) half[0] = E29::pack(acc);
    __syncthreads();
    if (wave == 0 && vl == 0) {
        acc = E29::add_quad(acc, E29::unpack(half[0]), q);
        if (q == 0) out[RED_ROWS + (blockIdx.x - RED_ROWS / 2)] = E29::pack(acc);
    }
}

// sum_j j * X_j = sum_{j>=1} Suffix_j with Suffix_j = sum_{i>=j} X_i: an inclusive suffix scan and a tree sum, both
// log-depth in LDS, over 128 elements with one QUAD per element (512 threads).  grid = (3, batch):
//   block 0: A' = sum_a a * (R_2a + R_2a+1)     (the 256 row sums taken in pairs; drop Suffix_0)
//   block 1: B  = sum_lo (lo+1) * C_lo          (keep Suffix_0)
//   block 2: Z  = sum_a R_2a+1                  (plain tree sum)
//   block 3: T  = sum_lo C_lo                   (plain tree sum; wide windows only: the segment's unweighted total)
// since sum_hi hi R_hi = 2 A' + Z, the host finishes  S = RED_COLS * (2 A' + Z) + B.   out[gridDim.x * m + which] = A', B, Z (, T)
template <class C>
__global__ void SRS_KERNEL_BOUNDS(RED_THREADS, 1)
    k_reduce_final(const xyzz_t *__restrict__ rc, xyzz_t *__restrict__ out) {
    constexpr uint32_t N = RED_COLS;                       // 128 elements per block
    using E29 = Ec29<C>;
    __shared__ xyzz29_t v[N];                              // lazy 9-limb coordinates: packing (two products) only for the final store
    const uint32_t m = blockIdx.y, t = threadIdx.x >> 2, q = threadIdx.x & 3u, which = blockIdx.x;
    const xyzz_t *rows = rc + (size_t)m * (RED_ROWS + RED_COLS), *cols = rows + RED_ROWS;
    xyzz29_t x;
    if (which == 0) x = E29::add_quad(E29::unpack(rows[2 * t]), E29::unpack(rows[2 * t + 1]), q);
    else if (which == 1 || which == 3) x = E29::unpack(cols[t]);
    else x = E29::unpack(rows[2 * t + 1]);
    if (which < 2) {
        if (q == 0) v[t] = x;
        __syncthreads();
        for (uint32_t s = 1; s < N; s <<= 1) {             // suffix scan
            const bool has = t + s < N;
            xyzz29_t o = has ? v[t + s] : E29::identity();
            __syncthreads();
            if (has) x = E29::add_quad(x, o, q);
            if (q == 0) v[t] = x;
            __syncthreads();
        }
        if (which == 0 && t == 0) x = E29::identity();
    }
    if (q == 0) v[t] = x;
    __syncthreads();
    for (uint32_t s = N >> 1; s >= 1; s >>= 1) {           // tree sum
        if (t < s) {                                       // x is kept in registers by all 4 lanes: the quad's own
            x = E29::add_quad(x, v[t + s], q);             // slot is never re-read, so lane 0's store cannot race with it
            if (q == 0) v[t] = x;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) out[(size_t)m * gridDim.x + which] = E29::pack(v[0]);
}

// wide windows: the 4 x NSEG_W partial sums of the segments -> 4 points.  A', B, Z add up (the bucket reduction is linear);
// bucket (v, lo) has weight v * NBUCKET + lo + 1, so the segment totals enter as U = sum_v v T_v (suffix sums, as above),
// which the host multiplies by NBUCKET.   grid = 1, block = 256: wavefront `which`, quad v
template <class C>
__global__ void SRS_KERNEL_BOUNDS(256, 1)
    k_wide_combine(const xyzz_t *__restrict__ in /* [NSEG_W][4] */, xyzz_t *__restrict__ out /* [4] */) {
    using E29 = Ec29<C>;
    const uint32_t which = threadIdx.x >> 6, lane = threadIdx.x & 63u, q = lane & 3u, vl = lane >> 2;
    xyzz29_t x = E29::unpack(in[vl * 4 + which]);
    if (which == 3) {
        for (uint32_t s = 1; s < NSEG_W; s <<= 1) {        // suffix scan over the 16 quads
            xyzz29_t o = shfl_down_point29(x, 4 * s, 64);
            if (vl + s < NSEG_W) x = E29::add_quad(x, o, q);
        }
        if (vl == 0) x = E29::identity();
    }
    for (unsigned d = NSEG_W / 2; d >= 1; d >>= 1) {
        xyzz29_t o = shfl_down_point29(x, 4 * d, 64);
        if (vl < d) x = E29::add_quad(x, o, q);
    }
    if (lane == 0) out[which] = E29::pack(x);
}

// the batched plain flow: the 3 sums of segment (j, w), packed by member, -> the landing layout, member slot[j] at point 3 NWIN slot[j]
// (where the single flows land it: finish_t reads either the same way).   grid = 1
struct LandMap {
    uint8_t slot[BATCH_ARGS];
};
__global__ void SRS_KERNEL_BOUNDS(256, 1)
    k_land_spread(const xyzz_t *__restrict__ in /* [members][nwin][3] */, xyzz_t *__restrict__ out /* [BATCH_ARGS][NWIN][3] */, LandMap map,
                  uint32_t members, uint32_t nwin) {
    for (uint32_t i = threadIdx.x; i < members * nwin * 3; i += blockDim.x) {
        const uint32_t j = i / (3 * nwin), r = i % (3 * nwin);
        out[3 * NWIN * (uint32_t)map.slot[j] + r] = in[i];
    }
}

// ---------------------------------------------------------------------------------------------
// key expansion and table upkeep (host side)
// ---------------------------------------------------------------------------------------------
static inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }

// windows 1 .. nwin-1 of a table whose window 0 (the bases, ABI form) is in place; `nbits` doublings between windows
template <class C>
static void expand_windows(affine_t *table, uint32_t n, int nwin, int nbits, xyzz_t *tmp, hipStream_t stream) {
    for (int w = 1; w < nwin; ++w) {
        const affine_t *prev = table + (size_t)(w - 1) * n;
        affine_t *cur = table + (size_t)w * n;
        SRS_LAUNCH((k_table_step<C>), (ceil_div(n, 256)), (256), 0, stream, prev, tmp, n, nbits);
        SRS_LAUNCH((k_normalize<C>), (ceil_div(ceil_div(n, NORM_G), 128)), (128), 0, stream, (const xyzz_t *)tmp, cur, n);
    }
}

// Which keys carry the second, 13-window table.  r03 ended with the wide pipeline opt-in: ahead at >= 12 M scalars (2^24 uniform 20.5 vs
// 22.5 ms) but with ONE full bench in which the row-program kernels ran slower on that box.  r04 repeated the comparison (three full
// benches each way on one box, profiles/r04_ab_wide_vs_narrow.txt): the anomaly did not come back -- the k = 20 step is the same with
// and without the second table (11.52 / 11.52 vs 11.55 / 11.57 ms), the 2^24 MSM is 19.9-20.0 vs 22.3 ms uniform and 10.30 vs 10.71 ms
// trace-like.  So: keys of >= 2^WIDE_MIN_KEY_LOG bases get the table (+81 % key memory: 29 GiB instead of 16 at 2^24) and WHOLE,
// device-resident MSMs of >= 2^WIDE_MIN_N_LOG scalars take the 20-bit windows; the sets of a streamed commit stay on the 16-bit windows
// and the slots (their chunks are 0.3-3 M scalars, where the wide pipeline's fixed costs lose).  SRS_MSM_WIDE=0 / 1: never / every key.
static bool wants_wide_table(size_t len) {
    // tuning msm_wide; unset: the environment's SRS_MSM_WIDE (a deployer's memory switch: 0 = no second table), else by key size
    static const int env_forced = [] { const char *e = std::getenv("SRS_MSM_WIDE"); return e ? std::atoi(e) : -1; }();
    const int forced = (int)tuning::get_or(tuning::MSM_WIDE, env_forced);
    if (forced == 0 || len == 0) return false;
    return forced == 1 || len >= ((size_t)1 << WIDE_MIN_KEY_LOG);
}

template <class C>
static void build_table_t(Key &k, hipStream_t stream) {
    const uint32_t n = (uint32_t)k.len;
    if (k.table_w) {
        SRS_HIP_CHECK(hipFree(k.table_w));
        k.table_w = nullptr;
    }
    if (n == 0) return;
    if (k.plain) {                           // the bases alone: no further window, no second table, only the table's coordinate form
        SRS_LAUNCH((k_table_form<C>), (ceil_div(n, 256)), (256), 0, stream, k.table, (size_t)n);
        SRS_HIP_CHECK(hipStreamSynchronize(stream));
        return;
    }
    xyzz_t *tmp = nullptr;
    SRS_HIP_CHECK(hipMalloc((void **)&tmp, (size_t)n * sizeof(xyzz_t)));
    // the second table is an optimisation (+81 % key memory): a device that cannot hold it keeps the 16-bit windows for everything
    // (use_wide() is false without table_w; srs_ck_has_wide_table tells).  A compact key created under msm_compact = 1 is the memory-saving
    // form: it never has one.  Under msm_compact = 2 it takes the table by the same rule as a full key, with 7 windows instead of 13 (a half
    // of the split scalar is below 2^126).
    const int nwin_w = k.compact ? NWIN_WC : NWIN_W;
    if ((!k.compact || k.compact_wide) && wants_wide_table(n) &&
        hipMalloc((void **)&k.table_w, (size_t)n * nwin_w * sizeof(affine_t)) != hipSuccess) {
        (void)hipGetLastError();
        k.table_w = nullptr;
    }
    if (k.table_w) {
        SRS_HIP_CHECK(hipMemcpyAsync(k.table_w, k.table, (size_t)n * sizeof(affine_t), hipMemcpyDeviceToDevice, stream));
        expand_windows<C>(k.table_w, n, nwin_w, WBITS_W, tmp, stream);
        const size_t total_w = (size_t)n * nwin_w;
        SRS_LAUNCH((k_table_form<C>), (ceil_div(total_w, 256)), (256), 0, stream, k.table_w, total_w);
    }
    const int nwin = k.compact ? NWIN_COMPACT : NWIN;
    expand_windows<C>(k.table, n, nwin, WBITS, tmp, stream);
    const size_t total = (size_t)n * nwin;
    SRS_LAUNCH((k_table_form<C>), (ceil_div(total, 256)), (256), 0, stream, k.table, total);
    SRS_HIP_CHECK(hipStreamSynchronize(stream));
    SRS_HIP_CHECK(hipFree(tmp));
}

template <class C>
static void generate_t(Key &k, uint64_t seed, hipStream_t stream) {
    const uint32_t n = (uint32_t)k.len;
    if (n == 0) return;
    xyzz_t *tmp = nullptr;
    SRS_HIP_CHECK(hipMalloc((void **)&tmp, (size_t)n * sizeof(xyzz_t)));
    SRS_LAUNCH((k_gen_bases<C>), (ceil_div(n, 128)), (128), 0, stream, tmp, n, seed, k.rank, k.world);
    SRS_LAUNCH((k_normalize<C>), (ceil_div(ceil_div(n, NORM_G), 128)), (128), 0, stream, (const xyzz_t *)tmp, k.table, n);
    SRS_HIP_CHECK(hipStreamSynchronize(stream));
    SRS_HIP_CHECK(hipFree(tmp));
}
void generate_bases(Key &k, uint64_t seed, hipStream_t stream) {
    if (k.curve == 0) generate_t<Bn256>(k, seed, stream); else generate_t<Grumpkin>(k, seed, stream);
}

size_t count_off_curve(const Key &k, hipStream_t stream) {
    if (k.len == 0) return 0;
    uint32_t *d_bad = nullptr, bad = 0;
    SRS_HIP_CHECK(hipMalloc((void **)&d_bad, sizeof(uint32_t)));
    SRS_HIP_CHECK(hipMemsetAsync(d_bad, 0, sizeof(uint32_t), stream));
    const uint32_t n = (uint32_t)k.len;
    if (k.curve == 0) SRS_LAUNCH((k_on_curve<Bn256>), (ceil_div(n, 256)), (256), 0, stream, (const affine_t *)k.table, n, d_bad);
    else SRS_LAUNCH((k_on_curve<Grumpkin>), (ceil_div(n, 256)), (256), 0, stream, (const affine_t *)k.table, n, d_bad);
    SRS_HIP_CHECK(hipMemcpyAsync(&bad, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    SRS_HIP_CHECK(hipStreamSynchronize(stream));
    (void)hipFree(d_bad);
    return bad;
}

void read_bases(const Key &k, affine_t *out_dev, hipStream_t stream) {
    if (k.len == 0) return;
    if (k.curve == 0) SRS_LAUNCH((k_table_unform<Bn256>), (ceil_div(k.len, 256)), (256), 0, stream, (const affine_t *)k.table, out_dev, k.len);
    else SRS_LAUNCH((k_table_unform<Grumpkin>), (ceil_div(k.len, 256)), (256), 0, stream, (const affine_t *)k.table, out_dev, k.len);
}

void build_table(Key &k, hipStream_t stream) {
    if (k.curve == 0) build_table_t<Bn256>(k, stream); else build_table_t<Grumpkin>(k, stream);
}

int choose_windows(Key &k) {
    const int64_t mode = tuning::get_or(tuning::MSM_COMPACT, 0);
    const int64_t form = tuning::get_or(tuning::MSM_PLAIN, 0);
    k.plain_form = (form == 1 || form == 2) ? (uint8_t)form : 0;
    k.plain = k.plain_form != 0;
    if (k.plain && mode != 0) {
        set_error("msm_plain = " + std::to_string(form) + " and msm_compact = " + std::to_string(mode) + " are both set: a key is plain (the bases alone) or compact (8 windows), choose one");
        throw DeviceError{4};      // SRS_ERR_INVALID
    }
    if (k.plain && k.world > 1) {
        set_error("plain key (msm_plain = " + std::to_string(form) + "): a key spread over " + std::to_string(k.world) + " ranks or devices is not supported");
        throw DeviceError{4};
    }
    if (k.plain) return 1;
    k.compact = mode == 1 || mode == 2;
    k.compact_wide = mode == 2;              // may carry the 7-window wide table (build_table: wants_wide_table)
    // the largest index, NWIN_COMPACT * len - 1, must lie below the endomorphism flag of an entry (the wide table's NWIN_WC * len - 1 is
    // smaller).  A guard: every creation entry already refuses keys above 2^27 bases (capi.hip), and 8 x 2^27 = 2^30 still fits, so this
    // cannot fire while that limit stands.
    static_assert(NWIN_WC <= NWIN_COMPACT, "choose_windows: the guard covers the wide table's payloads");
    if (k.compact && (uint64_t)NWIN_COMPACT * k.len > PAY_ENDO) {
        set_error("compact key (msm_compact = 1 / 2): 8 x " + std::to_string(k.len) + " table entries do not fit below the endomorphism flag (2^30)");
        throw DeviceError{4};      // SRS_ERR_INVALID
    }
    return k.compact ? NWIN_COMPACT : NWIN;
}
size_t table_bytes(const Key &k) {
    if (!k.table) return 0;
    if (k.plain) return k.len * sizeof(affine_t);
    return k.len * sizeof(affine_t) * ((k.compact ? NWIN_COMPACT : NWIN) + (k.table_w ? (k.compact ? NWIN_WC : NWIN_W) : 0));
}

// ---- host driver: three flows (16-bit windows with levels / in slot mode, wide windows) over shared stages -----------------------

// gathered mixed additions per level-0 thread.  Two losses pull in opposite directions: every part leaves a partial sum the
// later levels combine with the dearer full additions (+ 1.4 / L0 of the level-0 work), and the launch ends with a
// partly filled last wave of workgroups (the chip holds 2^18 level-0 threads at a time: + ~0.5 / waves, waves = entries /
// (L0 * 2^18)).  16 is best up to ~10 M scalars (measured on the chunks of a 12 * 2^20 commit: 64 cost 0.9 ms more in
// k_accum0 than it saved in k_accum1), 32 above, 64 from ~40 M.  Tuning msm_l0 = <log2> forces a value (tests).
static uint32_t l0_log_for(uint64_t M) {
    const int forced = (int)tuning::get_or(tuning::MSM_L0, 0);
    if (forced >= 1 && forced <= 7) return (uint32_t)forced;
    // small MSMs (the support circuit's 3 * 2^15 and 2^15-row commits) cannot fill the chip with 16-entry parts: 2^21 digit slots give
    // < 2^17 level-0 threads, each a chain of 16 dependent additions on a chip that holds 2^17.6 -- shorter parts, more threads (r03)
    // r05: parts of 8 from 2^20 digit slots on (was 2^21): the support circuit's batch (3 * 2^15 + 2 x 2^15 scalars, 1.6 M slots) 589 -> 501 us per call,
    // profiles/r05_ab_small_msm.txt -- with parts of 4 its first accumulation level has 5 partial sums per bucket to combine, with 8 two or three
    if (M < (1ull << 20)) return 2;
    if (M < (1ull << 22)) return 3;
    uint32_t lg = ACC_L0_LOG;
    while (lg < 7 && (M >> (lg + 1)) >= (5ull << 20)) ++lg;
    return lg;
}

// k_accum1 gives every output to a quad of lanes while a level has at most this many outputs (x batch): a level that cannot
// fill the chip's 2^17.6 resident lanes is a chain of dependent additions, and a quad shortens each by 3.3x for 1.3x the
// lane-cycles.  Tuning msm_quad_max = <log2> overrides (tests).
static uint32_t acc1_quad_max() {
    const int64_t lg = tuning::get_or(tuning::MSM_QUAD_MAX, 0);
    return (lg >= 1 && lg <= 24) ? (1u << lg) : ACC1_QUAD_MAX;
}

// number of thread-sequential levels, level 0 included, so that the wavefront-level final pass sees at most ~FINAL_FANIN parts
// per bucket even if every entry fell into one bucket (`parts`: the level-0 parts of that bucket)
static int levels_for(uint64_t parts) {
    int levels = 1;
    while (parts > FINAL_FANIN && levels < MAX_LEVELS) {
        parts = (parts + ACC_L1 - 1) / ACC_L1;
        ++levels;
    }
    return levels;
}

// large MSMs take the two-pass scatter (k_group + k_scatter2); tuning msm_sort = 1 / 2 forces the single- / two-pass path
static bool use_two_pass(uint64_t M, uint32_t batch) {
    const int forced = (int)tuning::get_or(tuning::MSM_SORT, 0);
    if (forced == 1) return false;
    if (forced == 2) return true;
    return M * batch >= TWO_PASS_MIN_SLOTS;
}

static uint32_t slot_log() {
    const int64_t lg = tuning::get_or(tuning::MSM_SLOT_LOG, 0);
    return (lg >= 2 && lg <= 8) ? (uint32_t)lg : SLOT_LOG;
}
// the part length a large set prefers when its buckets would fit shorter parts: 2^4
static uint32_t slot_want_cap() { return 4u; }

// ---- shapes: what the sizes, grids and kernel arguments of a set of launches follow from.  Every tunable-dependent choice is read
// ONCE per workspace_bytes* / enqueue call, into the shape; everything downstream takes it from there. ---------------------------------
struct LevelShape {            // every flow
    uint64_t M;                // digit slots = entry capacity (per MSM of a batch)
    int levels;                // accumulation levels incl. level 0 (slot mode: of the parts beyond the slots)
    size_t plan_stride;        // plan words per MSM / segment
    uint64_t cap0, cap1;       // points in ping = level-0 threads (= parts, worst case) and in pong = parts after level 1 (per MSM of a batch)
    uint32_t quad_max;         // acc1_quad_max()
};
struct SetShape : LevelShape { // the two flows of the 16-bit windows: + their counting sort
    bool two_pass;
    uint32_t tile, tiles;      // scalars per workgroup of k_hist / k_group / k_scatter, workgroups per window
};
struct NarrowShape : SetShape { uint32_t l0_log; };         // log2 of the part length (slot mode chooses it on the device: k_plan_s)
struct SlotShape : SetShape { uint32_t S, nred; };          // slots per bucket; reduction levels at the end of a commit (8 inputs per output)
struct WideShape : LevelShape { uint32_t l0_log, T, tiles_g; };   // log2 of the part length; workgroups of the segment passes, of the sort inside the segments (M = n x the key's digit rows)

static void sort_shape(SetShape &h, uint32_t n_max, uint32_t batch) {
    h.M = (uint64_t)n_max * NWIN;
    h.quad_max = acc1_quad_max();
    h.two_pass = use_two_pass(h.M, batch);
    // tile = digits per workgroup: large enough that the fixed 2^15-bin zero/scan of the LDS histogram is
    // amortised, small enough to give ~SORT_TARGET_BLOCKS workgroups (one per CU, 128 KiB LDS each)
    h.tile = (uint32_t)((h.M * batch + SORT_TARGET_BLOCKS - 1) / SORT_TARGET_BLOCKS);
    h.tile = (h.tile + 1023u) & ~1023u;
    if (h.tile < SORT_TILE_MIN) h.tile = SORT_TILE_MIN;
    h.tiles = ceil_div(n_max, h.tile);
}
static NarrowShape narrow_shape(uint32_t n_max, uint32_t batch) {
    NarrowShape h;
    sort_shape(h, n_max, batch);
    h.l0_log = l0_log_for(h.M);
    h.levels = levels_for((h.M + (1ull << h.l0_log) - 1) >> h.l0_log);
    h.plan_stride = (size_t)(h.levels + 1) * (NBUCKET + 1) + 4;
    h.cap0 = (h.M >> h.l0_log) + NBUCKET + 1;
    h.cap1 = h.cap0 / ACC_L1 + NBUCKET + 1;
    return h;
}
static SlotShape slot_shape(uint32_t n_max, uint32_t batch) {
    SlotShape h;
    sort_shape(h, n_max, batch);
    const uint32_t lg = slot_log();
    h.S = 1u << lg;
    h.nred = (lg + 2) / 3;
    // parts = sum_b ceil(c_b / L0) <= E / L0 + NBUCKET, and k_plan_s picks L0 >= (mean load) / (S - 1): never more than NBUCKET * S parts;
    // L0 >= 2^SLOT_L0_MIN_LOG bounds them for small sets
    h.cap0 = std::min<uint64_t>((uint64_t)NBUCKET * h.S, (h.M >> SLOT_L0_MIN_LOG) + NBUCKET);
    h.cap1 = h.cap0 / ACC_L1 + NBUCKET + 1;
    h.levels = levels_for(h.cap0);
    h.plan_stride = (size_t)(h.levels + 2) * (NBUCKET + 1) + 4;
    return h;
}
static WideShape wide_shape(uint32_t n, uint32_t digits /* rows per scalar: wide_digits(key is compact) */) {
    WideShape w;
    w.M = (uint64_t)n * digits;
    w.quad_max = acc1_quad_max();
    w.l0_log = l0_log_for(w.M);
    // worst case: every entry in one bucket of one segment.  That also bounds the hot top windows of a compact key (each half's seventh
    // digit is at most 2^6, so 2 of the 14 rows fall into <= 65 buckets of segment 0: n / 32 entries per bucket for uniform scalars, against
    // the 14 n this is sized for): k_plan finds <= FINAL_FANIN parts left for the wave-level pass within these levels
    w.levels = levels_for((w.M + (1ull << w.l0_log) - 1) >> w.l0_log);
    w.plan_stride = (size_t)(w.levels + 1) * (NBUCKET + 1) + 4;
    w.cap0 = (w.M >> w.l0_log) + (uint64_t)NSEG_W * (NBUCKET + 1);
    w.cap1 = w.cap0 / ACC_L1 + (uint64_t)NSEG_W * (NBUCKET + 1);
    w.T = ceil_div(n, WIDE_TILE);
    w.tiles_g = SORT_TARGET_BLOCKS;                          // the tile size is chosen on the device (k_seg_scan) so that this many suffice
    return w;
}

// ---- workspace: every flow lists its buffers ONCE, as a walk over a "walker" -- the Sizer, which adds up what the arena would hand out
// (workspace_bytes*, so reserve()), or the Arena, which hands it out (enqueue).  reserve() must be right for a LATER enqueue (growing the
// arena mid-commit would free memory still in use): one list per flow cannot disagree with itself, and carve() checks it. ---------------
struct Sizer {
    size_t used = 0;
    template <class T>
    T *take(size_t count) {
        used += Arena::pad(count * sizeof(T));
        return nullptr;
    }
};
template <class Walk>
static size_t sized(Walk walk) {
    Sizer s;
    walk(s);
    return s.used;
}
template <class Walk>
static auto carve(Arena &A, Walk walk) {
    const size_t need = sized(walk);
    A.reserve(need);
    A.reset();
    const auto bufs = walk(A);
    if (A.used != need) {
        set_error("internal: msm workspace: the arena walk and the sizer disagree");
        throw DeviceError{5};
    }
    return bufs;
}

struct SetBufs {               // what both flows of the 16-bit windows carve, each x batch
    xyzz_t *d_out, *ping, *pong, *rc;              // the 3 partial sums per MSM; partial sums of the levels; row / column sums
    uint16_t *dig, *tb;                            // digits; thread -> bucket map of level 0
    uint32_t *sorted, *count, *cursor, *plan;
    uint16_t *gkey;                                // two-pass scatter only: grouped keys / payloads, per-tile segment counts
    uint32_t *gpay, *tile_hist;
};
struct NarrowBufs : SetBufs { xyzz_t *buckets; };
struct SlotBufs : SetBufs { xyzz_t *red_a, *red_b; };       // ping / pong of the slot reduction
// head and tail of both lists: sort_front() reads either flow through SetBufs, so the common buffers are taken in one place
template <class W>
static void take_set_head(W &A, const SetShape &h, uint32_t batch, SetBufs &b) {
    b.d_out = A.template take<xyzz_t>(3 * (size_t)batch);
    b.dig = A.template take<uint16_t>(h.M * batch);
    b.sorted = A.template take<uint32_t>(h.M * batch);
    b.count = A.template take<uint32_t>((size_t)NBUCKET * batch);
    b.cursor = A.template take<uint32_t>((size_t)NBUCKET * batch);
    b.plan = A.template take<uint32_t>(h.plan_stride * batch);
    b.ping = A.template take<xyzz_t>(h.cap0 * batch);                      // slot mode: the parts beyond the slots
    b.tb = A.template take<uint16_t>(h.cap0 * batch);
    b.pong = A.template take<xyzz_t>(h.cap1 * batch);
}
template <class W>
static void take_set_tail(W &A, const SetShape &h, uint32_t batch, SetBufs &b) {
    b.rc = A.template take<xyzz_t>((size_t)(RED_ROWS + RED_COLS) * batch);
    b.gkey = h.two_pass ? A.template take<uint16_t>(h.M * batch) : nullptr;
    b.gpay = h.two_pass ? A.template take<uint32_t>(h.M * batch) : nullptr;
    b.tile_hist = h.two_pass ? A.template take<uint32_t>((size_t)SEG * (SORT_TARGET_BLOCKS + 2 * NWIN) * batch) : nullptr;
}
template <class W>
static NarrowBufs narrow_layout(W &A, const NarrowShape &h, uint32_t batch) {
    NarrowBufs b;
    take_set_head(A, h, batch, b);
    b.buckets = A.template take<xyzz_t>((size_t)NBUCKET * batch);
    take_set_tail(A, h, batch, b);
    return b;
}
template <class W>
static SlotBufs slot_layout(W &A, const SlotShape &h, uint32_t batch) {
    SlotBufs b;
    take_set_head(A, h, batch, b);
    b.red_a = A.template take<xyzz_t>((size_t)NBUCKET * (h.S / 8 + 1) * batch);
    b.red_b = A.template take<xyzz_t>((size_t)NBUCKET * (h.S / 64 + 1) * batch);
    take_set_tail(A, h, batch, b);
    return b;
}
template <uint32_t NS = NSEG_W>
struct WideBufsT {
    xyzz_t *d_out, *d_seg, *ping, *pong, *buckets, *rc;     // the MSM's 4 sums; 4 per segment; as in SetBufs, for the 16 segments together
    uint16_t *gkey, *gkey2, *tb;                   // grouped by segment (MSD pass), and again by sub-segment: the counting sort inside the
    uint32_t *gpay, *gpay2, *tile_cnt, *tile_hist; // segments in two passes through LDS (k_group_g + k_scatter2_g); their per-tile counts
    uint32_t *seg3;                                // seg_total, seg_off, tile_base, tile_base2: NSEG_W + 2 words each
    uint32_t *sorted, *count, *cursor, *plan;
    LinkT<NS> *link;
};
using WideBufs = WideBufsT<>;
template <class W>
static WideBufs wide_layout(W &A, const WideShape &w) {
    WideBufs b;
    b.d_out = A.template take<xyzz_t>(4);
    b.d_seg = A.template take<xyzz_t>(4 * NSEG_W);
    b.gkey = A.template take<uint16_t>(w.M);
    b.gpay = A.template take<uint32_t>(w.M);
    b.sorted = A.template take<uint32_t>(w.M);
    b.tile_cnt = A.template take<uint32_t>((size_t)NSEG_W * w.T);
    b.gkey2 = A.template take<uint16_t>(w.M);
    b.gpay2 = A.template take<uint32_t>(w.M);
    b.tile_hist = A.template take<uint32_t>((size_t)SEG * w.tiles_g);
    b.seg3 = A.template take<uint32_t>(4 * (NSEG_W + 2));
    b.link = A.template take<Link>(1);
    b.count = A.template take<uint32_t>((size_t)NSEG_W * NBUCKET);
    b.cursor = A.template take<uint32_t>((size_t)NSEG_W * NBUCKET);
    b.plan = A.template take<uint32_t>(w.plan_stride * NSEG_W);
    b.ping = A.template take<xyzz_t>(w.cap0);
    b.tb = A.template take<uint16_t>(w.cap0);
    b.pong = A.template take<xyzz_t>(w.cap1);
    b.buckets = A.template take<xyzz_t>((size_t)NSEG_W * NBUCKET);
    b.rc = A.template take<xyzz_t>((size_t)NSEG_W * (RED_ROWS + RED_COLS));
    return b;
}

size_t workspace_bytes(uint32_t n_max, uint32_t batch) {
    return sized([&](auto &A) { return narrow_layout(A, narrow_shape(n_max, batch), batch); });
}
static size_t workspace_bytes_slots(uint32_t n_max, uint32_t batch) {
    return sized([&](auto &A) { return slot_layout(A, slot_shape(n_max, batch), batch); });
}
static size_t workspace_bytes_wide(uint32_t n, uint32_t digits) {
    return sized([&](auto &A) { return wide_layout(A, wide_shape(n, digits)); });
}

// ---- shared stages --------------------------------------------------------------------------------------------------------------
// Sort front end of the 16-bit windows: scalars -> digits -> histogram -> the flow's plan (`launch_plan`: k_plan / k_plan_s) -> the
// (bucket, table-index) pairs sorted by bucket, in one pass or two, and the thread -> bucket map of plan array `arr` in b.tb.
// `group_maps`: the two-pass sort's k_group writes that map as well (k_expand's work), so that k_expand runs only after the single pass.
template <class C, class LaunchPlan>
static void sort_front(const Key &k, const SetShape &h, const SetBufs &b, const fe_t *const *scalars_dev, const uint32_t *n_host,
                       const uint32_t *base_host, uint32_t batch, uint32_t n_max, int is_mont, hipStream_t stream, LaunchPlan launch_plan,
                       bool group_maps, uint32_t arr) {
    BatchDesc bd;
    for (uint32_t m = 0; m < BATCH_ARGS; ++m) {
        bd.ptr[m] = m < batch ? scalars_dev[m] : nullptr;
        bd.n[m] = m < batch ? n_host[m] : 0;
        bd.base[m] = (m < batch && base_host) ? base_host[m] : 0;
    }
    const uint32_t s_rank = k.compact_scalars ? 0u : k.rank, s_world = k.compact_scalars ? 1u : k.world;
    const size_t M = (size_t)h.M;
    // a compact key differs in three kernels of this stage -- the split digits and the payload line of either scatter -- and in level 0
    const auto digits = k.compact ? &k_digits<C, true> : &k_digits<C, false>;
    const auto group = k.compact ? &k_group<true> : &k_group<false>;
    const auto scatter = k.compact ? &k_scatter<true> : &k_scatter<false>;
    SRS_LAUNCH(digits, (ceil_div(n_max, 256), batch), (256), 0, stream, bd, b.dig, M, is_mont, s_rank, s_world, b.count,
               (uint32_t)(NBUCKET * batch));
    SRS_LAUNCH(k_hist, (h.tiles, NWIN, batch), (SORT_THREADS), 0, stream, (const uint16_t *)b.dig, M, bd, b.count, h.tile, b.tile_hist);
    launch_plan();
    if (h.two_pass) {
        const uint32_t T1 = h.tiles * NWIN;
        SRS_LAUNCH(k_scan_seg, (SEG, batch), (1024), 0, stream, b.tile_hist, T1, (const uint32_t *)b.plan, h.plan_stride);
        SRS_LAUNCH(group, (h.tiles, NWIN, batch), (SORT_THREADS), 0, stream, (const uint16_t *)b.dig, M, bd, (const uint32_t *)b.tile_hist,
                   b.gkey, b.gpay, M, (uint32_t)k.len, h.tile, group_maps ? (const uint32_t *)b.plan : nullptr,
                   group_maps ? h.plan_stride : (size_t)0, group_maps ? b.tb : nullptr, group_maps ? (size_t)h.cap0 : (size_t)0,
                   group_maps ? arr : 0u);
        // 8 x ceil(tiles / 8) workgroups: the XCD-aware mapping of k_scatter2 needs every (XCD, slot) pair to exist
        SRS_LAUNCH(k_scatter2, (8 * ceil_div(ceil_div(M, SORT_TILE2), 8), batch), (SORT_THREADS), 0, stream, (const uint16_t *)b.gkey,
                   (const uint32_t *)b.gpay, M, (const uint32_t *)b.plan, h.plan_stride, b.cursor, b.sorted, M, (uint32_t)SORT_TILE2);
    } else {
        SRS_LAUNCH(scatter, (h.tiles, NWIN, batch), (SORT_THREADS), 0, stream, (const uint16_t *)b.dig, M, bd, b.cursor, b.sorted, M,
                   (uint32_t)k.len, h.tile);
    }
    if (!(h.two_pass && group_maps))
        SRS_LAUNCH(k_expand<>, (NBUCKET / 4, batch), (256), 0, stream, (const uint32_t *)b.plan, h.plan_stride, b.tb, (size_t)h.cap0,
                   (const Link *)nullptr, arr);
}

// what the level kernels and the bucket reduction read of a set: its plan and the partial sums of the levels, ping (even levels) and
// pong, with their strides per MSM of the batch -- 0 with a link: the segments of the wide flow share the buffers
template <uint32_t NS = NSEG_W>
struct PartsT {
    const uint32_t *plan; size_t plan_stride;
    xyzz_t *ping; size_t stride0;
    xyzz_t *pong; size_t stride1;
    const LinkT<NS> *link;
};
using Parts = PartsT<>;

// accumulation levels 1 .. levels - 1 over ping / pong; `cap_inc`: what a level's worst-case part count adds to an eighth of the previous one
template <class C, uint32_t NS = NSEG_W>
static void accum_levels(const PartsT<NS> &p, const LevelShape &h, uint64_t cap_inc, uint32_t batch, hipStream_t stream) {
    xyzz_t *cur = p.ping, *nxt = p.pong;
    size_t cur_stride = p.stride0, nxt_stride = p.stride1;
    uint64_t cap = h.cap0;
    for (int level = 1; level < h.levels; ++level) {
        cap = cap / ACC_L1 + cap_inc;
        SRS_LAUNCH((k_accum1<C, NS>), (ceil_div(std::max<uint64_t>(cap, 4 * std::min<uint64_t>(cap, h.quad_max)), ACC_THREADS), batch),
                   (ACC_THREADS), 0, stream, (const xyzz_t *)cur, cur_stride, p.plan, h.plan_stride, level, nxt, nxt_stride, (uint32_t)ACC_L1,
                   p.link, h.quad_max);
        std::swap(cur, nxt);
        std::swap(cur_stride, nxt_stride);
        // both buffers can hold any later level: parts shrink monotonically and pong >= level-1 cap
    }
}

// bucket reduction of `nmsm` MSMs / segments: row and column sums (k_rowcol: of `from`, or with from_buckets == 0 of `from` plus what
// the plan left in ping / pong), then their `sums` weighted totals per MSM into d_sums
template <class C, uint32_t NS = NSEG_W>
static void reduce_buckets(const PartsT<NS> &p, uint32_t nmsm, const xyzz_t *from, int from_buckets, xyzz_t *rc, uint32_t sums, xyzz_t *d_sums,
                           hipStream_t stream) {
    SRS_LAUNCH((k_rowcol<C, NS>), (RED_ROWS / 2 + RED_COLS, nmsm), (128), 0, stream, from, (const xyzz_t *)p.ping, p.stride0,
               (const xyzz_t *)p.pong, p.stride1, p.plan, p.plan_stride, rc, p.link, from_buckets);
    SRS_LAUNCH((k_reduce_final<C>), (sums, nmsm), (RED_THREADS), 0, stream, (const xyzz_t *)rc, d_sums);
}

// points of one landing slot: 3 partial sums per MSM -- per WINDOW of every MSM on a plain key
static size_t landing_pts(const Key &k) { return 3 * (size_t)BATCH_ARGS * (k.plain ? NWIN : 1); }
// a set's `n` partial sums into landing slot `slot` (page-locked host memory) from its point `at` on, in stream order
static void land(Key &k, const xyzz_t *d_out, size_t n, uint32_t slot, hipStream_t stream, size_t at = 0) {
    if (!k.h_result) SRS_HIP_CHECK(hipHostMalloc(&k.h_result, landing_pts(k) * LANDING_SLOTS * sizeof(xyzz_t)));
    xyzz_t *dst = static_cast<xyzz_t *>(k.h_result) + landing_pts(k) * slot + at;
    SRS_HIP_CHECK(hipMemcpyAsync(dst, d_out, n * sizeof(xyzz_t), hipMemcpyDeviceToHost, stream));
}

// ---- the level flow of the 16-bit windows ---------------------------------------------------------------------------------------
// launches one set of <= BATCH_ARGS MSMs on `stream`; the 3 partial sums of MSM m land in landing slot `slot`
// (page-locked host memory) in stream order.  Returns false when every MSM is empty (nothing was launched).
template <class C>
static bool enqueue_t(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, const uint32_t *base_host, uint32_t batch,
                      uint32_t n_max, int is_mont, hipStream_t stream, uint32_t slot, Fold fold) {
    if (n_max == 0) return false;
    const NarrowShape h = narrow_shape(n_max, batch);
    const NarrowBufs b = carve(k.arena, [&](auto &A) { return narrow_layout(A, h, batch); });
    sort_front<C>(k, h, b, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, [&] {
        SRS_LAUNCH(k_plan, (batch, h.levels + 1), (PLAN_THREADS), 0, stream, (const uint32_t *)b.count, b.cursor, b.plan, h.plan_stride,
                   h.levels, h.l0_log, (uint32_t)ACC_L1_LOG, (const uint32_t *)nullptr);
    }, false, 1u);
    const Parts p{b.plan, h.plan_stride, b.ping, (size_t)h.cap0, b.pong, (size_t)h.cap1, nullptr};
    const uint64_t units = std::accumulate(n_host, n_host + batch, (uint64_t)0);
    const auto accum0 = k.compact ? &k_accum0c<C> : &k_accum0<C>;
    SRS_LAUNCH_TIMED("msm_accum0", units, accum0, (ceil_div(h.cap0, ACC_THREADS), batch), (ACC_THREADS), 0, stream,
                     (const uint32_t *)b.sorted, (size_t)h.M, p.plan, p.plan_stride, (const uint16_t *)b.tb, p.stride0,
                     (const affine_t *)k.table, p.ping, p.stride0, 1u << h.l0_log, p.link);
    accum_levels<C>(p, h, NBUCKET + 1, batch, stream);
    SRS_LAUNCH((k_accum_final<C>), (NBUCKET / (FINAL_THREADS / 64), batch), (FINAL_THREADS), 0, stream, (const xyzz_t *)p.ping, p.stride0,
               (const xyzz_t *)p.pong, p.stride1, p.plan, p.plan_stride, b.buckets, p.link);
    const xyzz_t *red_from = b.buckets;
    int from_buckets = 0;
    if (fold != FOLD_NONE) {
        if (!k.fold_buckets) SRS_HIP_CHECK(hipMalloc((void **)&k.fold_buckets, (size_t)NBUCKET * sizeof(xyzz_t)));
        SRS_LAUNCH((k_bucket_fold<C>), (NBUCKET / 64), (64), 0, stream, (const xyzz_t *)b.buckets, (const xyzz_t *)p.ping,
                   (const xyzz_t *)p.pong, p.plan, p.plan_stride, k.fold_buckets, fold == FOLD_FIRST ? 1 : 0);
        if (fold != FOLD_LAST) return true;                  // no reduction, no result for this set
        red_from = k.fold_buckets;
        from_buckets = 1;
    }
    reduce_buckets<C>(p, batch, red_from, from_buckets, b.rc, 3, b.d_out, stream);
    land(k, b.d_out, 3 * (size_t)batch, slot, stream);
    k.landing[slot].wide = false;
    return true;
}

static bool use_wide(const Key &k, uint32_t n_max, uint32_t batch);
// ---- slot mode ------------------------------------------------------------------------------------------------------------------
// Slot mode is for the sets of a CHUNKED commit (fold != FOLD_NONE): that is where every set used to pay its own accumulation levels, wave-level
// pass and bucket fold.  A set that is a whole MSM keeps the r03 flow, by measurement (profiles/r04_ab_slots_cuts.txt): the batched
// cross-term commitments would each pay a slot reduction (k = 17 Sangria step 6.02 vs 5.76 ms), a single 2^24 MSM is 2 % slower (22.3 vs
// 21.85 ms).  Tuning msm_slots = 0: never; 2: every 16-bit-window set (what the emulator tests force).
static bool use_slots(const Key &k, uint32_t n_max, uint32_t batch, Fold fold) {
    const int mode = (int)tuning::get_or(tuning::MSM_SLOTS, 1);
    if (mode == 0) return false;
    if (fold != FOLD_NONE) return batch == 1;
    return mode == 2 && !use_wide(k, n_max, batch);
}

// one set of <= BATCH_ARGS MSMs in slot mode.  fold: NONE = a whole commit (first and last set), FIRST / MIDDLE / LAST = the sets of a
// chunked commit (batch == 1): only the last one reduces the slots and lands the 3 partial sums.
template <class C>
static bool enqueue_slots_t(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, const uint32_t *base_host, uint32_t batch,
                            uint32_t n_max, int is_mont, hipStream_t stream, uint32_t slot, Fold fold) {
    if (n_max == 0) return false;
    const bool first = fold == FOLD_NONE || fold == FOLD_FIRST, last = fold == FOLD_NONE || fold == FOLD_LAST;
    const SlotShape h = slot_shape(n_max, batch);
    const uint32_t S = h.S;
    if (first) {
        k.slot_s = S;
        k.seq = 0;
        k.commit_ovf = k.expect_ovf;
        const size_t need = (size_t)batch * NBUCKET * S;
        if (k.slots_pts < need) {
            if (k.slots) SRS_HIP_CHECK(hipFree(k.slots));
            k.slots = nullptr;
            k.slots_pts = 0;
            SRS_HIP_CHECK(hipMalloc((void **)&k.slots, need * sizeof(xyzz_t)));
            k.slots_pts = need;
        }
        if (!k.used) SRS_HIP_CHECK(hipMalloc((void **)&k.used, 2 * (size_t)BATCH_ARGS * NBUCKET));
        if (!k.h_ovf) {
            SRS_HIP_CHECK(hipHostMalloc((void **)&k.h_ovf, 2 * (size_t)LANDING_SLOTS * BATCH_ARGS * sizeof(uint32_t)));
            for (size_t i = 0; i < 2 * (size_t)LANDING_SLOTS * BATCH_ARGS; ++i) k.h_ovf[i] = 0;
        }
    } else if (k.slot_s != S || batch != 1) {
        set_error("internal: msm slot mode: a commit's sets must share the slot layout");
        throw DeviceError{5};
    }
    const uint8_t *used_prev = k.used + (size_t)(k.seq & 1u) * BATCH_ARGS * NBUCKET;
    uint8_t *used_next = k.used + (size_t)((k.seq + 1) & 1u) * BATCH_ARGS * NBUCKET;
    ++k.seq;

    const SlotBufs b = carve(k.arena, [&](auto &A) { return slot_layout(A, h, batch); });
    const uint32_t arr = (uint32_t)h.levels + 1;             // the plan array of the level-0 parts
    sort_front<C>(k, h, b, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, [&] {
        SRS_LAUNCH(k_plan_s, (batch, h.levels + 2), (PLAN_THREADS), 0, stream, (const uint32_t *)b.count, b.cursor, b.plan, h.plan_stride,
                   h.levels, S, (uint32_t)ACC_L1_LOG, used_prev, used_next, first ? 1 : 0, k.h_ovf + (size_t)slot * BATCH_ARGS, slot_want_cap());
    }, true, arr);
    const Parts p{b.plan, h.plan_stride, b.ping, (size_t)h.cap0, b.pong, (size_t)h.cap1, nullptr};
    const uint64_t units = std::accumulate(n_host, n_host + batch, (uint64_t)0);
    const auto accum0s = k.compact ? &k_accum0sc<C> : &k_accum0s<C>;
    SRS_LAUNCH_TIMED("msm_accum0", units, accum0s, (ceil_div(h.cap0, ACC_THREADS), batch), (ACC_THREADS), 0, stream,
                     (const uint32_t *)b.sorted, (size_t)h.M, p.plan, p.plan_stride, arr, (const uint16_t *)b.tb, p.stride0,
                     (const affine_t *)k.table, k.slots, S, used_prev, first ? 1 : 0, p.ping, p.stride0);
    if (k.commit_ovf) {                      // hot buckets expected: the parts beyond the slots go through the level kernels into slot S - 1
        accum_levels<C>(p, h, NBUCKET + 1, batch, stream);
        SRS_LAUNCH((k_ovf_final<C>), (NBUCKET / (FINAL_THREADS / 64), batch), (FINAL_THREADS), 0, stream, (const xyzz_t *)p.ping, p.stride0,
                   (const xyzz_t *)p.pong, p.stride1, p.plan, p.plan_stride, k.slots, S, first ? 1 : 0);
    }
    k.landing[slot] = {false, true, k.commit_ovf, batch};
    ++k.stat_slot_sets;
    if (!last) return true;
    // the commit's one reduction: slots -> buckets (8 inputs per output and level), then the usual row / column sums
    const xyzz_t *in = k.slots;
    uint32_t in_pb = S;
    xyzz_t *outs[2] = {b.red_a, b.red_b};
    for (uint32_t l = 0; l < h.nred; ++l) {
        const uint32_t out_pb = (in_pb + 7) / 8, n_out = NBUCKET * out_pb;
        xyzz_t *out = outs[l & 1u];
        const uint8_t *used = l == 0 ? used_next : nullptr;
        const int extra = (l == 0 && k.commit_ovf) ? (int)S - 1 : -1;
        if (l + 1 == h.nred) {
            SRS_LAUNCH((k_slot_reduce<C, true>), (ceil_div((uint64_t)n_out * 4, 256), batch), (256), 0, stream, in, in_pb, used, (size_t)NBUCKET, extra,
                       out, out_pb);
        } else {
            SRS_LAUNCH((k_slot_reduce<C, false>), (ceil_div(n_out, 256), batch), (256), 0, stream, in, in_pb, used, (size_t)NBUCKET, extra, out,
                       out_pb);
        }
        in = out;
        in_pb = out_pb;
    }
    reduce_buckets<C>(p, batch, in, 1, b.rc, 3, b.d_out, stream);
    land(k, b.d_out, 3 * (size_t)batch, slot, stream);
    return true;
}

bool overflow_missed(const Key &k, uint32_t slot) {
    if (slot >= LANDING_SLOTS || !k.landing[slot].slot_mode || k.landing[slot].ovf_on || !k.h_ovf) return false;
    for (uint32_t m = 0; m < k.landing[slot].batch; ++m)
        if (k.h_ovf[(size_t)slot * BATCH_ARGS + m]) return true;
    return false;
}
void note_commit(Key &k, const uint32_t *slots_used, uint32_t n_slots, uint64_t scalars) {
    bool any = false, slot_sets = false;
    uint64_t entries = 0;
    for (uint32_t i = 0; i < n_slots; ++i) {
        const uint32_t sl = slots_used[i];
        if (sl >= LANDING_SLOTS || !k.landing[sl].slot_mode || !k.h_ovf) continue;
        slot_sets = true;
        for (uint32_t m = 0; m < k.landing[sl].batch; ++m) entries += k.h_ovf[(size_t)(LANDING_SLOTS + sl) * BATCH_ARGS + m];
        bool hot = false;
        for (uint32_t m = 0; m < k.landing[sl].batch; ++m) hot = hot || k.h_ovf[(size_t)sl * BATCH_ARGS + m] != 0;
        if (hot) ++k.stat_hot_sets;
        any = any || hot;
    }
    // hot buckets are expected at once -- and from a key's FIRST commit (r05: Key::expect_ovf starts true; a witness of 0 / 1 / small values is
    // the common case and its first commit used to run twice) -- and un-expected only after COLD_COMMITS commits in a row without them:
    // launching the overflow kernels for nothing costs ~0.3 ms of empty launches per commit, missing them costs the commit run a second time
    constexpr uint32_t COLD_COMMITS = 3;
    if (!slot_sets) {                        // no slot-mode set: no entry count either -- the next commit's cuts fall back to the default schedule
        k.last_entries = k.last_scalars = 0;
        return;
    }
    k.last_entries = entries;
    k.last_scalars = scalars;
    if (any) {
        k.expect_ovf = true;
        k.cold_streak = 0;
    } else if (k.expect_ovf && ++k.cold_streak >= COLD_COMMITS) {
        k.expect_ovf = false;
        k.cold_streak = 0;
    }
}

// ---- the wide-window pipeline: ONE MSM of n >= 2^WIDE_MIN_N_LOG scalars over table_w -------------------------------------
static bool use_wide(const Key &k, uint32_t n_max, uint32_t batch) {
    const int min_log = (int)tuning::get_or(tuning::MSM_WIDE_MIN, (int64_t)WIDE_MIN_N_LOG);
    return k.table_w != nullptr && batch == 1 && n_max >= (1u << min_log);
}

// The flow of the 16 segments, shared by the wide windows and by plain keys: segment counts -> offsets -> grouping (the two passes of
// `seg_count` / `seg_group` over the scalars), the counting sort inside the segments, level 0 over `table`, the levels and the bucket
// reduction of the 16 segments as ONE linked batch -> `sums` partial sums per segment in b.d_seg.
// `nseg`: the segments that can hold an entry, 0 .. nseg - 1 (a plain key of form 2: 8).  The plan, the maps, the wave-level pass and the
// bucket reduction run for these alone.  The stages in front only see segments without entries: k_seg_scan gives them no tile (tile_base
// and tile_base2 repeat the total, so link_segment stays below nseg) and k_link no part.
// `reduce` = false stops behind k_accum_final (a folded set of a plain key: its buckets go into the key's running buckets instead); the
// parts of the linked batch are returned for whoever goes on.
template <class C>
struct SegKernels {
    decltype(&k_seg_pass<C, false, false>) seg_count, seg_group;
    decltype(&k_group_g<false>) group_g;
    decltype(&k_accum0<C>) accum0;
};
// The flow for a segment capacity NS (NSEG_W, or PLAIN_BATCH_SEG in the batched plain flow, whose segments are the (member, window)
// pairs of a set).  `front(group)` launches the segment pass over the scalars (group = false: counts, true: grouping) on w.T
// workgroups; `scan_rows`: the rows of tile_cnt, one workgroup of k_seg_scan each; `units`: the scalars (the timing record of level 0).
template <class C, uint32_t NS, class Front>
static PartsT<NS> segment_flow_core(const WideShape &w, const WideBufsT<NS> &b, Front front, decltype(&k_group_g<false, NS>) group_g,
                                    decltype(&k_accum0<C, NS>) accum0, uint64_t units, const affine_t *table, uint32_t sums,
                                    hipStream_t stream, uint32_t nseg, uint32_t scan_rows, bool reduce) {
    uint32_t *seg_total = b.seg3, *seg_off = b.seg3 + (NS + 2), *tile_base = b.seg3 + 2 * (NS + 2), *tile_base2 = b.seg3 + 3 * (NS + 2);
    // sort: segment counts -> offsets -> grouping (MSD pass), then the counting sort inside the segments
    SRS_HIP_CHECK(hipMemsetAsync(seg_total, 0, (NS + 1) * sizeof(uint32_t), stream));
    SRS_HIP_CHECK(hipMemsetAsync(b.count, 0, (size_t)nseg * NBUCKET * sizeof(uint32_t), stream));
    front(false);
    const uint32_t small_tiles = (w.M >> 19) < 64 ? 1u : 0u, tile2_host = small_tiles ? SORT_TILE2 / 4 : SORT_TILE2;
    SRS_LAUNCH(k_seg_scan<NS>, (scan_rows), (1024), 0, stream, b.tile_cnt, w.T, (const uint32_t *)seg_total, seg_off, tile_base, tile_base2, small_tiles);
    front(true);
    SRS_LAUNCH(k_hist_g<NS>, (w.tiles_g), (SORT_THREADS), 0, stream, (const uint16_t *)b.gkey, (const uint32_t *)seg_off,
               (const uint32_t *)tile_base, b.count, b.tile_hist);
    SRS_LAUNCH(k_plan, (nseg, w.levels + 1), (PLAN_THREADS), 0, stream, (const uint32_t *)b.count, b.cursor, b.plan, w.plan_stride, w.levels,
               w.l0_log, (uint32_t)ACC_L1_LOG, (const uint32_t *)seg_off);
    SRS_LAUNCH(k_scan_seg_g, (SEG, nseg), (1024), 0, stream, b.tile_hist, w.tiles_g, (const uint32_t *)tile_base, (const uint32_t *)b.plan,
               w.plan_stride);
    SRS_LAUNCH(group_g, (w.tiles_g), (SORT_THREADS), 0, stream, (const uint16_t *)b.gkey, (const uint32_t *)b.gpay, (const uint32_t *)seg_off,
               (const uint32_t *)tile_base, (const uint32_t *)b.tile_hist, b.gkey2, b.gpay2);
    // tiles of SORT_TILE2 entries cut per segment: at most M / SORT_TILE2 + (segments in use) of them; 8 x ceil(. / 8) workgroups (XCD mapping)
    SRS_LAUNCH(k_scatter2_g<NS>, (8 * ceil_div(ceil_div(w.M, tile2_host) + scan_rows, 8)), (SORT_THREADS), 0, stream, (const uint16_t *)b.gkey2,
               (const uint32_t *)b.gpay2, (const uint32_t *)seg_off, (const uint32_t *)tile_base2, b.cursor, b.sorted);
    SRS_LAUNCH(k_link<NS>, (1), (NS > 64 ? NS : 64), 0, stream, (const uint32_t *)b.plan, w.plan_stride, w.levels, b.link, nseg);
    // from here on the segments are ONE linked batch: no strides, the link says where a segment's parts start
    const PartsT<NS> p{b.plan, w.plan_stride, b.ping, 0, b.pong, 0, b.link};
    SRS_LAUNCH(k_expand<NS>, (NBUCKET / 4, nseg), (256), 0, stream, p.plan, p.plan_stride, b.tb, (size_t)0, p.link, 1u);
    SRS_LAUNCH_TIMED("msm_accum0", units, accum0, (ceil_div(w.cap0, ACC_THREADS)), (ACC_THREADS), 0, stream, (const uint32_t *)b.sorted,
                     (size_t)0, p.plan, p.plan_stride, (const uint16_t *)b.tb, (size_t)0, table, p.ping, (size_t)0,
                     1u << w.l0_log, p.link);
    accum_levels<C, NS>(p, w, (uint64_t)nseg * (NBUCKET + 1), 1, stream);
    SRS_LAUNCH((k_accum_final<C, NS>), (NBUCKET / (FINAL_THREADS / 64), nseg), (FINAL_THREADS), 0, stream, (const xyzz_t *)p.ping, p.stride0,
               (const xyzz_t *)p.pong, p.stride1, p.plan, p.plan_stride, b.buckets, p.link);
    if (reduce) reduce_buckets<C, NS>(p, nseg, b.buckets, 0, b.rc, sums, b.d_seg, stream);
    return p;
}
template <class C>
static Parts segment_flow(const WideShape &w, const WideBufs &b, const WideDesc &wd, uint32_t table_stride, const SegKernels<C> &kn,
                          const affine_t *table, uint32_t sums, hipStream_t stream, uint32_t nseg = NSEG_W, bool reduce = true) {
    uint32_t *seg_total = b.seg3;
    const auto front = [&](bool group) {
        if (!group)
            SRS_LAUNCH(kn.seg_count, (w.T), (WIDE_THREADS), 0, stream, wd, b.tile_cnt, w.T, seg_total, (uint16_t *)nullptr,
                       (uint32_t *)nullptr, table_stride);
        else
            SRS_LAUNCH(kn.seg_group, (w.T), (WIDE_THREADS), 0, stream, wd, b.tile_cnt, w.T, seg_total, b.gkey, b.gpay, table_stride);
    };
    return segment_flow_core<C, NSEG_W>(w, b, front, kn.group_g, kn.accum0, wd.n, table, sums, stream, nseg, NSEG_W, reduce);
}

template <class C>
static bool enqueue_wide_t(Key &k, const fe_t *scalars_dev, uint32_t n, uint32_t base, int is_mont, hipStream_t stream, uint32_t slot) {
    const WideShape w = wide_shape(n, wide_digits(k.compact));
    // a compact key differs in the two segment passes (split digits, 14 rows, flagged payloads), in the hot sub-segment of k_group_g and in level 0
    const SegKernels<C> kn = k.compact ? SegKernels<C>{&k_seg_pass<C, false, true>, &k_seg_pass<C, true, true>, &k_group_g<true>, &k_accum0c<C>}
                                       : SegKernels<C>{&k_seg_pass<C, false, false>, &k_seg_pass<C, true, false>, &k_group_g<false>, &k_accum0<C>};
    const WideBufs b = carve(k.arena, [&](auto &A) { return wide_layout(A, w); });
    const WideDesc wd{scalars_dev, n, base, k.compact_scalars ? 0u : k.rank, k.compact_scalars ? 1u : k.world, is_mont};
    segment_flow<C>(w, b, wd, (uint32_t)k.len, kn, k.table_w, 4, stream);
    SRS_LAUNCH((k_wide_combine<C>), (1), (256), 0, stream, (const xyzz_t *)b.d_seg, b.d_out);
    land(k, b.d_out, 4, slot, stream);
    k.landing[slot].wide = true;
    return true;
}

// ---- the plain flow: ONE MSM of any size over a plain key (window 0 alone) ------------------------------------------------------------
// The wide flow (segment_flow) with the WINDOW as the segment: k_seg_pass<PLAIN> groups the 16 n signed 16-bit digits by window, and from
// k_hist_g to reduce_buckets the 16 windows are the 16 linked segments -- every entry gathers from k.table, the bases.  What leaves is 3 partial sums
// per window, landed at point 3 NWIN m of the slot; finish_t weights the windows.  A set of two or more MSMs runs as ONE such flow over
// (member, window) segments (the batched plain flow, below); where it does not (use_plain_batch), MSM m of the set is one flow after the
// other on the stream: they share the arena in stream order (the caller has reserved it for the largest of them).
// Form 2 (msm_plain = 2, Key::plain_form): the same flow over the split scalar.  k_seg_pass<PLAIN, GLV> leaves 2 entries per scalar in
// each of 8 windows, those of k2 flagged PAY_ENDO; level 0 is k_accum0c, which multiplies a flagged entry's x by beta; the stages from the
// plan on run for 8 segments (segment_flow: nseg), 3 x 8 partial sums land and finish_t weights 8 windows.  A scalar has 16 digit rows in
// either form, so the shape, the buffers and workspace_bytes_plain are those of form 1.
static WideShape plain_shape(uint32_t n) { return wide_shape(n, NWIN); }
static int plain_windows(int form) { return form == 2 ? NWIN_COMPACT : NWIN; }
// what the flows of up to n_max scalars need.  The layout grows with n while the part length stays (wide_shape), but a longer part shrinks
// ping / pong: the largest n of every shorter part length is a candidate too, so that a smaller MSM later on the stream never grows the arena
static size_t workspace_bytes_plain(uint32_t n_max) {
    size_t need = 0;
    for (uint32_t n = n_max; n;) {
        need = std::max(need, sized([&](auto &A) { return wide_layout(A, plain_shape(n)); }));
        const uint32_t lg = l0_log_for((uint64_t)n * NWIN);
        uint32_t lo = 1, hi = n;                               // smallest count with this part length
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (l0_log_for((uint64_t)mid * NWIN) == lg) hi = mid; else lo = mid + 1;
        }
        n = lo - 1;
    }
    return need;
}

template <class C>
static void enqueue_plain_t(Key &k, const fe_t *scalars_dev, uint32_t n, uint32_t base, int is_mont, hipStream_t stream, uint32_t slot,
                            uint32_t m, Fold fold = FOLD_NONE) {
    const WideShape w = plain_shape(n);
    const SegKernels<C> kn = k.plain_form == 2
        ? SegKernels<C>{&k_seg_pass<C, false, false, true, true>, &k_seg_pass<C, true, false, true, true>, &k_group_g<false>, &k_accum0c<C>}
        : SegKernels<C>{&k_seg_pass<C, false, false, true>, &k_seg_pass<C, true, false, true>, &k_group_g<false>, &k_accum0<C>};
    const WideBufs b = carve(k.arena, [&](auto &A) { return wide_layout(A, w); });
    const WideDesc wd{scalars_dev, n, base, 0u, 1u, is_mont};            // a plain key is never sharded (choose_windows)
    const uint32_t nwin = (uint32_t)plain_windows(k.plain_form);
    if (fold != FOLD_NONE) {                                             // a set of a chunked commit: the window is the bucket set, whatever the base offset
        const Parts p = segment_flow<C>(w, b, wd, 0u, kn, k.table, 3, stream, nwin, false);
        if (!k.fold_buckets) SRS_HIP_CHECK(hipMalloc((void **)&k.fold_buckets, (size_t)nwin * NBUCKET * sizeof(xyzz_t)));
        SRS_LAUNCH((k_bucket_fold_seg<C>), (NBUCKET / 64, nwin), (64), 0, stream, (const xyzz_t *)b.buckets, (const xyzz_t *)p.ping,
                   (const xyzz_t *)p.pong, p.plan, p.plan_stride, p.link, k.fold_buckets, fold == FOLD_FIRST ? 1 : 0);
        ++k.stat_plain_fold_sets;
        if (fold != FOLD_LAST) return;                                   // no reduction, no result for this set
        reduce_buckets<C>(p, nwin, k.fold_buckets, 1, b.rc, 3, b.d_seg, stream);
        ++k.stat_plain_reductions;
        land(k, b.d_seg, 3 * (size_t)nwin, slot, stream);
        return;
    }
    segment_flow<C>(w, b, wd, 0u, kn, k.table, 3, stream, nwin);
    ++k.stat_plain_reductions;
    land(k, b.d_seg, 3 * (size_t)nwin, slot, stream, 3 * (size_t)NWIN * m);     // (the slot keeps room for 16 windows per MSM in either form)
}

// ---- the batched plain flow: the MSMs of ONE set as one linked flow ------------------------------------------------------------------
// The segment is the pair (member j, window w) -- j counts the set's non-empty members --, global index j * windows + w, S = members x
// windows of them (<= PLAIN_BATCH_SEG = 256).  k_seg_pass_b groups every member's digits by (member, window) in one launch over the flat
// tile space of all members; from k_seg_scan on the S segments are what the 16 windows are to one MSM: one plan, one link, one level 0
// and one set of levels over a flat thread space in which the parts of every member balance, one wave-level pass, one bucket reduction
// of S segments, one landing copy.  All kernels that see more than 16 segments are the NS = PLAIN_BATCH_SEG instantiations.
// A set stays sequential (enqueue_plain_t per member, as before): under tuning msm_plain_batch = 0, with one non-empty member, when
// its 16 x sum n_m digit slots would not fit the 32-bit entry offsets, when it folds, and above PLAIN_BATCH_MAX_N scalars in a member.
// Measured (profiles/plain_batch_ab.txt): the batched flow is faster at every member size of the sweep, 5 x 2^12 .. 5 x 2^20 and
// 16 x 2^12, on both forms (by 38-50 % at 2^12, 17-23 % at 2^15, 7-10 % at 2^20), so no size inside the sweep stays sequential; sets
// with a larger member were not measured and do.
// Workspace: per segment 4 MiB of buckets, 4 MiB of level-0 parts and 4 MiB of level-1 parts (an empty bucket owns one part on every
// level), the plan (0.25 MiB per level) and 0.25 MiB of counts and cursors, about 13 MiB -- 1.0 GiB for 5 members on form 1, 3.4 GiB
// at 256 segments; part of the key's grow-only arena (reserve()), not of table_bytes().
constexpr uint32_t PLAIN_BATCH_MAX_N = 1u << 20;
struct PlainBatchShape : WideShape { uint32_t S; };
// `n_sum`, `n_max`: all the scalars of the set and those of its largest member; T: tiles over all members
static PlainBatchShape plain_batch_shape(uint64_t n_sum, uint32_t n_max, uint32_t T, uint32_t S) {
    PlainBatchShape w;
    w.S = S;
    w.M = n_sum * NWIN;
    w.quad_max = acc1_quad_max();
    const uint64_t m_max = (uint64_t)n_max * NWIN;           // what a segment can hold: the part length and the levels follow the largest member,
    w.l0_log = l0_log_for(m_max);                            // as in its own flow (worst case: its entries in one bucket of one segment)
    w.levels = levels_for((m_max + (1ull << w.l0_log) - 1) >> w.l0_log);
    w.plan_stride = (size_t)(w.levels + 1) * (NBUCKET + 1) + 4;
    w.cap0 = (w.M >> w.l0_log) + (uint64_t)S * (NBUCKET + 1);        // an empty bucket owns one (identity) part on every level
    w.cap1 = w.cap0 / ACC_L1 + (uint64_t)S * (NBUCKET + 1);
    w.T = T;
    w.tiles_g = SORT_TARGET_BLOCKS - NSEG_W + S;             // k_seg_scan: that many full tiles, one partly filled per segment
    return w;
}
struct PlainBatchBufs : WideBufsT<PLAIN_BATCH_SEG> { xyzz_t *d_land; };
template <class W>
static PlainBatchBufs plain_batch_layout(W &A, const PlainBatchShape &w) {
    constexpr uint32_t NS = PLAIN_BATCH_SEG;
    PlainBatchBufs b;
    b.d_out = nullptr;
    b.d_land = A.template take<xyzz_t>(3 * (size_t)NWIN * BATCH_ARGS);
    b.d_seg = A.template take<xyzz_t>(3 * (size_t)w.S);
    b.gkey = A.template take<uint16_t>(w.M);
    b.gpay = A.template take<uint32_t>(w.M);
    b.sorted = A.template take<uint32_t>(w.M);
    b.tile_cnt = A.template take<uint32_t>((size_t)w.S * w.T);
    b.gkey2 = A.template take<uint16_t>(w.M);
    b.gpay2 = A.template take<uint32_t>(w.M);
    b.tile_hist = A.template take<uint32_t>((size_t)SEG * w.tiles_g);
    b.seg3 = A.template take<uint32_t>(4 * (NS + 2));
    b.link = A.template take<LinkT<NS>>(1);
    b.count = A.template take<uint32_t>((size_t)w.S * NBUCKET);
    b.cursor = A.template take<uint32_t>((size_t)w.S * NBUCKET);
    b.plan = A.template take<uint32_t>(w.plan_stride * w.S);
    b.ping = A.template take<xyzz_t>(w.cap0);
    b.tb = A.template take<uint16_t>(w.cap0);
    b.pong = A.template take<xyzz_t>(w.cap1);
    b.buckets = A.template take<xyzz_t>((size_t)w.S * NBUCKET);
    b.rc = A.template take<xyzz_t>((size_t)w.S * (RED_ROWS + RED_COLS));
    return b;
}
static bool plain_batch_on() { return tuning::get_or(tuning::MSM_PLAIN_BATCH, 1) != 0; }
// the members a batched set may carry at n_max scalars each: BATCH_ARGS, fewer where 16 x sum n_m would reach 2^32; 0: none
static uint32_t plain_batch_members(uint32_t n_max, uint32_t batch) {
    if (n_max == 0 || n_max > PLAIN_BATCH_MAX_N) return 0;
    const uint64_t fit = ((1ull << 32) - 1) / ((uint64_t)NWIN * n_max);
    const uint32_t b = (uint32_t)std::min<uint64_t>(std::min<uint32_t>(batch, BATCH_ARGS), fit);
    return b >= 2 ? b : 0;
}
// what a batched set of up to `batch` members of up to n_max scalars needs: every size grows with the members and their scalars while
// the part length stays; as in workspace_bytes_plain the largest n of every shorter part length is a candidate too
static size_t workspace_bytes_plain_batch(uint32_t n_max, uint32_t batch, int form) {
    size_t need = 0;
    for (uint32_t n = std::min(n_max, PLAIN_BATCH_MAX_N); n;) {
        const uint32_t b = plain_batch_members(n, batch);
        if (b)
            need = std::max(need, sized([&](auto &A) {
                return plain_batch_layout(A, plain_batch_shape((uint64_t)b * n, n, b * ceil_div(n, WIDE_TILE), b * (uint32_t)plain_windows(form)));
            }));
        const uint32_t lg = l0_log_for((uint64_t)n * NWIN);
        uint32_t lo = 1, hi = n;                               // smallest count with this part length
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (l0_log_for((uint64_t)mid * NWIN) == lg) hi = mid; else lo = mid + 1;
        }
        n = lo - 1;
    }
    return need;
}
// does this set take the batched flow?  (read per set: tuning msm_plain_batch)
static bool use_plain_batch(const uint32_t *n_host, uint32_t batch, Fold fold) {
    if (fold != FOLD_NONE || !plain_batch_on()) return false;
    uint32_t members = 0, n_max = 0;
    uint64_t n_sum = 0;
    for (uint32_t m = 0; m < batch; ++m) {
        members += n_host[m] ? 1u : 0u;
        n_max = std::max(n_max, n_host[m]);
        n_sum += n_host[m];
    }
    return members >= 2 && n_max <= PLAIN_BATCH_MAX_N && n_sum * NWIN < (1ull << 32);
}

template <class C>
static uint32_t enqueue_plain_batch_t(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, const uint32_t *base_host, uint32_t batch,
                                      int is_mont, hipStream_t stream, uint32_t slot) {
    constexpr uint32_t NS = PLAIN_BATCH_SEG;
    const bool glv = k.plain_form == 2;
    const uint32_t nwin = (uint32_t)plain_windows(k.plain_form);
    PlainBatchDesc bd{};
    LandMap map{};
    uint32_t members = 0, T = 0, n_max = 0, ran = 0, last = 0;
    uint64_t n_sum = 0;
    for (uint32_t m = 0; m < batch; ++m) {
        if (n_host[m] == 0) continue;
        bd.ptr[members] = scalars_dev[m];
        bd.n[members] = n_host[m];
        bd.base[members] = base_host ? base_host[m] : 0u;
        bd.tile0[members] = T;
        map.slot[members] = (uint8_t)m;
        T += ceil_div(n_host[m], WIDE_TILE);
        n_max = std::max(n_max, n_host[m]);
        n_sum += n_host[m];
        ran |= 1u << m;
        last = m;
        ++members;
    }
    for (uint32_t j = members; j <= BATCH_ARGS; ++j) bd.tile0[j] = T;
    bd.is_mont = is_mont;
    const uint32_t S = members * nwin;
    const PlainBatchShape w = plain_batch_shape(n_sum, n_max, T, S);
    const PlainBatchBufs b = carve(k.arena, [&](auto &A) { return plain_batch_layout(A, w); });
    SRS_HIP_CHECK(hipMemsetAsync(b.tile_cnt, 0, (size_t)S * T * sizeof(uint32_t), stream));   // a row holds counts at its member's tiles alone
    const auto front = [&](bool group) {
        const auto pass = glv ? (group ? &k_seg_pass_b<C, true, true> : &k_seg_pass_b<C, false, true>)
                              : (group ? &k_seg_pass_b<C, true, false> : &k_seg_pass_b<C, false, false>);
        SRS_LAUNCH(pass, (T), (WIDE_THREADS), 0, stream, bd, b.tile_cnt, T, b.seg3, group ? b.gkey : (uint16_t *)nullptr,
                   group ? b.gpay : (uint32_t *)nullptr);
    };
    segment_flow_core<C, NS>(w, b, front, &k_group_g<false, NS>, glv ? &k_accum0c<C, NS> : &k_accum0<C, NS>, n_sum, k.table, 3, stream, S, S,
                             true);
    SRS_LAUNCH(k_land_spread, (1), (256), 0, stream, (const xyzz_t *)b.d_seg, b.d_land, map, members, nwin);
    land(k, b.d_land, 3 * (size_t)NWIN * (last + 1), slot, stream);
    k.stat_plain_reductions += members;
    ++k.stat_plain_batch_sets;
    k.stat_plain_batch_msms += members;
    return ran;
}

// a set of <= BATCH_ARGS MSMs on a plain key.  Returns false when every MSM is empty (nothing was launched).
template <class C>
static bool enqueue_plain_set_t(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, const uint32_t *base_host, uint32_t batch,
                                int is_mont, hipStream_t stream, uint32_t slot, Fold fold) {
    uint32_t n_max = 0, ran = 0;
    for (uint32_t m = 0; m < batch; ++m) n_max = std::max(n_max, n_host[m]);
    if (n_max == 0) return false;
    const bool batched = use_plain_batch(n_host, batch, fold);
    if (batched) {
        ran = enqueue_plain_batch_t<C>(k, scalars_dev, n_host, base_host, batch, is_mont, stream, slot);
    } else {
        k.arena.reserve(workspace_bytes_plain(n_max));      // before the first launch: growing it between two flows would free memory in use
        for (uint32_t m = 0; m < batch; ++m) {
            if (n_host[m] == 0) continue;
            enqueue_plain_t<C>(k, scalars_dev[m], n_host[m], base_host ? base_host[m] : 0u, is_mont, stream, slot, m, fold);
            ran |= 1u << m;
        }
    }
    k.landing[slot].plain_batched = batched;
    k.landing[slot].wide = false;
    k.landing[slot].plain = true;
    k.landing[slot].plain_form = k.plain_form;
    k.landing[slot].plain_ran = ran;
    return true;
}

static ParallelFor g_parallel_for = nullptr;
void set_parallel_for(ParallelFor pf) { g_parallel_for = pf; }

// host end of enqueue_t, after `stream` has been synchronised:  S = RED_COLS * (2 A' + Z) + B  (10 group operations per MSM)
template <class C>
static void finish_t(Key &k, uint32_t batch, uint32_t slot, bool launched, xyzz_t *result_host) {
    if (!launched) {
        for (uint32_t m = 0; m < batch; ++m) result_host[m] = Ec<C>::identity();
        return;
    }
    const xyzz_t *raw = static_cast<const xyzz_t *>(k.h_result) + landing_pts(k) * slot;
    // the device sums arrive in the R' = 2^261 form of the 29-bit multiplier: times 2^-5 (as a Montgomery product) -> ABI form
    using F = typename C::F;
    fe_t c = F::one();
    for (int d = 0; d < 5; ++d) c = F::halve(c);
    const bool plain = k.landing[slot].plain;
    const int nwin = plain_windows(plain ? k.landing[slot].plain_form : 0);    // windows a plain flow landed per MSM
    std::vector<xyzz_t> two(plain ? 3 * (size_t)NWIN * batch : 3 * (size_t)batch + (k.landing[slot].wide ? 1 : 0));
    for (size_t i = 0; i < two.size(); ++i) {
        if (plain && (i / 3) % NWIN >= (size_t)nwin) continue;  // form 2 lands 8 of the 16 windows an MSM has room for
        two[i].x = F::mul(raw[i].x, c);
        two[i].y = F::mul(raw[i].y, c);
        two[i].zz = F::mul(raw[i].zz, c);
        two[i].zzz = F::mul(raw[i].zzz, c);
    }
    const auto bucket_sum = [&](size_t at) {                    // of the 3 partial sums from `at` on
        xyzz_t a = Ec<C>::add(Ec<C>::dbl(two[at]), two[at + 2]);
        for (uint32_t j = 1; j < RED_COLS; j <<= 1) a = Ec<C>::dbl(a);
        return Ec<C>::add(a, two[at + 1]);
    };
    if (plain) {                                                // sum_w 2^(16 w) R_w as a Horner chain from the top window: 240 doublings, 15 additions
        const auto chain = [&](size_t m) {                      // (form 2: 8 windows, 112 doublings, 8 additions)
            xyzz_t acc = Ec<C>::identity();
            for (int w = nwin - 1; w >= 0 && (k.landing[slot].plain_ran >> m & 1u); --w) {
                for (int d = 0; d < WBITS && w != nwin - 1; ++d) acc = Ec<C>::dbl(acc);
                acc = Ec<C>::add(acc, bucket_sum(3 * ((size_t)NWIN * m + w)));
            }
            result_host[m] = acc;
        };
        // the chains of the members do not depend on one another.  Behind a batched set they are the largest serial item left
        // (0.2-0.5 ms each on one core), so they go over the host workers the library keeps (set_parallel_for); tuning
        // msm_plain_batch = 2 keeps them on the calling thread (the A/B of profiles/plain_batch_ab.txt)
        if (k.landing[slot].plain_batched && g_parallel_for && tuning::get_or(tuning::MSM_PLAIN_BATCH, 1) != 2) {
            g_parallel_for(batch, chain);
            return;
        }
        for (uint32_t m = 0; m < batch; ++m) chain(m);
        return;
    }
    for (uint32_t m = 0; m < batch; ++m) result_host[m] = bucket_sum(3 * (size_t)m);
    if (k.landing[slot].wide) {                                 // one MSM, 4 sums: + NBUCKET * U for the segment totals
        xyzz_t u = two[3];
        for (uint32_t j = 1; j < NBUCKET; j <<= 1) u = Ec<C>::dbl(u);
        result_host[0] = Ec<C>::add(result_host[0], u);
    }
}

bool enqueue(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, const uint32_t *base_host, uint32_t batch, int is_mont,
             hipStream_t stream, uint32_t slot, Fold fold) {
    if (batch > BATCH_ARGS || slot >= LANDING_SLOTS) {
        set_error("internal: msm::enqueue batch / slot out of range");
        throw DeviceError{5};
    }
    if (fold != FOLD_NONE && batch != 1) {
        set_error("internal: msm::enqueue fold needs one MSM per set");
        throw DeviceError{5};
    }
    if (k.plain) {                           // every set, whatever its size: no slot mode, no wide table; a folded set adds into the running buckets
        if (fold != FOLD_NONE && n_host[0] == 0) {       // (its commit's result is the LAST set's: no set of it may drop out)
            set_error("internal: msm::enqueue empty folded set on a plain key");
            throw DeviceError{5};
        }
        k.landing[slot].slot_mode = false;
        ++k.stat_other_sets;
        return k.curve == 0 ? enqueue_plain_set_t<Bn256>(k, scalars_dev, n_host, base_host, batch, is_mont, stream, slot, fold)
                            : enqueue_plain_set_t<Grumpkin>(k, scalars_dev, n_host, base_host, batch, is_mont, stream, slot, fold);
    }
    if (batch == 1 && fold == FOLD_NONE && use_wide(k, n_host[0], 1)) {      // the sets of a chunked commit stay on the 16-bit windows
        const uint32_t base = base_host ? base_host[0] : 0;
        k.landing[slot].slot_mode = false;
        ++k.stat_other_sets;
        return k.curve == 0 ? enqueue_wide_t<Bn256>(k, scalars_dev[0], n_host[0], base, is_mont, stream, slot)
                            : enqueue_wide_t<Grumpkin>(k, scalars_dev[0], n_host[0], base, is_mont, stream, slot);
    }
    uint32_t n_max = 0;
    for (uint32_t m = 0; m < batch; ++m) n_max = std::max(n_max, n_host[m]);
    // the sets of one commit take the same flow: decided by its first set
    const bool first = fold == FOLD_NONE || fold == FOLD_FIRST;
    const bool slots = first ? use_slots(k, n_max, batch, fold) : k.slot_s != 0;
    if (slots)
        return k.curve == 0 ? enqueue_slots_t<Bn256>(k, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, slot, fold)
                            : enqueue_slots_t<Grumpkin>(k, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, slot, fold);
    if (first) k.slot_s = 0;
    k.landing[slot].slot_mode = false;
    ++k.stat_other_sets;
    return k.curve == 0 ? enqueue_t<Bn256>(k, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, slot, fold)
                        : enqueue_t<Grumpkin>(k, scalars_dev, n_host, base_host, batch, n_max, is_mont, stream, slot, fold);
}
void finish(Key &k, uint32_t batch, uint32_t slot, bool launched, xyzz_t *result_host) {
    if (k.curve == 0) finish_t<Bn256>(k, batch, slot, launched, result_host); else finish_t<Grumpkin>(k, batch, slot, launched, result_host);
}
void reserve(Key &k, uint32_t n_max, uint32_t batch) {
    if (k.plain) {                           // one arena: for the flow of one MSM (a sequential set runs its members one after the other) and,
        size_t b = workspace_bytes_plain(n_max);             // unless tuning msm_plain_batch = 0 keeps every set sequential, for the batched flow
        if (batch > 1 && plain_batch_on()) b = std::max(b, workspace_bytes_plain_batch(n_max, batch, k.plain_form));
        k.arena.reserve(b);
        return;
    }
    size_t b = use_wide(k, n_max, batch) ? std::max(workspace_bytes_wide(n_max, wide_digits(k.compact)), workspace_bytes(n_max, batch))
                                         : workspace_bytes(n_max, batch);
    if (batch == 1) b = std::max(b, workspace_bytes_slots(n_max, batch));        // (a chunked commit's sets: slot mode)
    k.arena.reserve(b);
}

void release(Key &k) {
    if (k.table_w) (void)hipFree(k.table_w);
    k.table_w = nullptr;
    if (k.fold_buckets) (void)hipFree(k.fold_buckets);
    k.fold_buckets = nullptr;
    if (k.h_result) (void)hipHostFree(k.h_result);
    k.h_result = nullptr;
    if (k.slots) (void)hipFree(k.slots);
    k.slots = nullptr;
    k.slots_pts = 0;
    if (k.used) (void)hipFree(k.used);
    k.used = nullptr;
    if (k.h_ovf) (void)hipHostFree(k.h_ovf);
    k.h_ovf = nullptr;
    k.arena.release();
}

void run(Key &k, const fe_t *const *scalars_dev, const uint32_t *n_host, uint32_t batch, int is_mont,
         hipStream_t stream, xyzz_t *result_host) {
    for (uint32_t at = 0; at < batch;) {                           // the batch descriptor is a kernel argument of BATCH_ARGS slots
        uint32_t b = std::min<uint32_t>(BATCH_ARGS, batch - at);
        if (use_wide(k, n_host[at], 1)) b = 1;                     // large vectors go through the wide-window pipeline one by one
        bool launched = enqueue(k, scalars_dev + at, n_host + at, nullptr, b, is_mont, stream, 0);
        if (launched) {
            SRS_HIP_CHECK(hipStreamSynchronize(stream));
            SRS_HIP_CHECK(hipGetLastError());
            const uint32_t sl = 0;
            if (overflow_missed(k, sl)) {                          // hot buckets the prediction did not expect: once more, with the overflow kernels
                k.expect_ovf = true;
                ++k.stat_redo;
                launched = enqueue(k, scalars_dev + at, n_host + at, nullptr, b, is_mont, stream, 0);
                SRS_HIP_CHECK(hipStreamSynchronize(stream));
                SRS_HIP_CHECK(hipGetLastError());
            }
            uint64_t total = 0;
            for (uint32_t m = 0; m < b; ++m) total += n_host[at + m];
            note_commit(k, &sl, 1, total);
        }
        finish(k, b, 0, launched, result_host + at);
        prof::collect();
        at += b;
    }
}

}  // namespace msm
}  // namespace srs
