// rowprog_dev.cuh -- device-side definitions shared by the ahead-of-time kernels in rowprog.hip and by the row programs
// compiled at run time with hiprtc (jit.hip embeds this file verbatim: keep it free of host-only includes).
#pragma once
#include "field.cuh"
#include "field29.cuh"
#include "lanes.cuh"      // SRS_SWEEP_ACC
#include "stripes.h"      // STRIPE_LOG, Stripes: rows are sharded like the key's entries

namespace srs {
namespace rowprog {

struct Insn {   // 16 bytes, read wave-uniformly
    uint32_t op, dst, a, b;
};

enum : uint32_t { I_LD_SEL = 0, I_LD_FIX, I_LD_ADV, I_ADD, I_SUB, I_MUL, I_SQR, I_DBL, I_NEG };
constexpr uint32_t UNIFORM_BIT = 0x80000000u;
constexpr uint32_t RP_THREADS = 128;
constexpr uint32_t DMAX = 8;   // cross terms kept in VGPRs per pass; higher degrees take ceil(d / 8) passes over the points
constexpr uint32_t DEGREE_LIMIT = 255;   // evaluation points 0..d must stay < 2^8 (small_times)

constexpr uint32_t JMAX = 16;  // witnesses combined by one advice load (cross terms: 2; ProtoGalaxy G: L + 1 <= 16)

// everything a row needs besides the program
struct RowCtx {
    uint32_t rows;
    const uint8_t *const *sel;
    const fe_t *const *fix;
    const fe_t *W[JMAX];      // column-major [num_advice][rows] each
    uint32_t J;               // number of witnesses
    const fe_t *wcoef;        // [npts][J] combination coefficients, or nullptr:
                              //   J == 1: W[0];  J == 2: W[0] + pt * W[1]  (cross-term points X = pt)
    uint32_t shard_rank, shard_world, local_rows;   // multi-GPU: this rank evaluates only the rows of ITS block-cyclic stripes
                              //   (2^STRIPE_LOG rows each, the stripes of the sharded commitment key); world == 1: all rows
    uint32_t half;            // J == 2, wcoef == nullptr: (W[0] + W[1]) / 2 + pt * (W[0] - W[1]) / 2, i.e. the Lagrange fold
                              //   L_0(X) W[0] + L_1(X) W[1] over the domain {1, -1} at the integer point X = pt (compute_G, L = 1)
    uint32_t pt0;             // sweep form only: the first evaluation point is X = pt0 instead of X = 0 (compute_G skips X = 1 when the
                              //   caller knows G(1) = F(alpha) and X = 0 with it: the points are 2 .. d + 1)
};

struct DevArgs {
    const Insn *prog;
    uint32_t n_insn;
    uint32_t result;          // operand code of the expression value
    RowCtx ctx;
    const fe_t *utab;         // [npts][n_uniform]
    uint32_t n_uniform;
    uint32_t npts;            // d + 1 (interpolate) or 1 (plain evaluation)
    uint32_t d;               // number of outputs in interpolate mode
    const fe_t *vinv;         // [d][npts]: T_k = sum_j vinv[(k-1)*npts + j] * P(j)
    const fe_t *vinv29;       // the same matrix * 2^5: operands of the 2^261-radix multiplier (sweep form)
    fe_t *const *out;         // d (interpolate) or 1 (plain) output vectors of `rows`
};

template <class F>
__device__ __forceinline__ fe_t small_times(const fe_t &x, uint32_t j) {   // j * x for a tiny j
    fe_t acc = F::zero();
    bool any = false;
    for (int b = j < 32u ? 4 : 7; b >= 0; --b) {
        if (any) acc = F::dbl(acc);
        if ((j >> b) & 1u) {
            acc = any ? F::add(acc, x) : x;
            any = true;
        }
    }
    return acc;
}

// One multiplier body per kernel for the straight-line programs (emit_spec_source): a program with every 2 KB multiplier
// inlined is hundreds of KB of code streamed once per evaluation point; called, it is tens of KB.
template <class F>
__device__ __attribute__((noinline)) fe_t mul_ni(fe_t a, fe_t b) { return F::mul(a, b); }
template <class F>
__device__ __attribute__((noinline)) fe_t sqr_ni(fe_t a) { return F::sqr(a); }

template <class F>
__device__ __attribute__((noinline)) f29_t mul29_ni(f29_t a, f29_t b SRS_F29_SITE) { return Fp29<typename F::Params>::mul(a, b SRS_F29_SITE_PASS); }
template <class F>
__device__ __attribute__((noinline)) f29_t sqr29_ni(f29_t a SRS_F29_SITE) { return Fp29<typename F::Params>::sqr(a SRS_F29_SITE_PASS); }

// column loads (PlonkEvalDomain::eval_column_var / eval_advice_var, src/plonk/eval.rs:57-69,153-228)
template <class F>
__device__ __forceinline__ fe_t ld_sel(const RowCtx &C, uint32_t col, uint32_t rr) { return C.sel[col][rr] ? F::one() : F::zero(); }
template <class F>
__device__ __forceinline__ fe_t ld_fix(const RowCtx &C, uint32_t col, uint32_t rr) { return C.fix[col][rr]; }
template <class F>
__device__ __forceinline__ fe_t ld_adv(const RowCtx &C, uint32_t col, uint32_t rr, uint32_t pt) {
    size_t idx = (size_t)col * C.rows + rr;
    if (C.wcoef == nullptr) {
        fe_t r = C.W[0][idx];
        if (C.J == 2 && C.half) {
            const fe_t w1 = C.W[1][idx];
            const fe_t a = F::halve(F::add(r, w1)), b = F::halve(F::sub(r, w1));
            return pt ? F::add(a, small_times<F>(b, pt)) : a;
        }
        if (C.J == 2 && pt) r = F::add(r, small_times<F>(C.W[1][idx], pt));
        return r;
    }
    const fe_t *cf = C.wcoef + (size_t)pt * C.J;
    fe_t r = F::mul(cf[0], C.W[0][idx]);
    for (uint32_t j = 1; j < C.J; ++j) r = F::add(r, F::mul(cf[j], C.W[j][idx]));
    return r;
}

// sweep form (rowprog_compile.hip, emit_sweep_source): an advice leaf as an affine function of the evaluation point,
// value(pt) = cur + pt * step.  Only for the point sets without a coefficient table (C.wcoef == nullptr):
//   J == 1: the witness itself;  J == 2: W[0] + pt W[1] (cross terms);  J == 2, half: the Lagrange fold at integer points.
template <class F>
__device__ __forceinline__ void adv_affine(const RowCtx &C, uint32_t col, uint32_t rr, fe_t &cur, fe_t &step) {
    const size_t idx = (size_t)col * C.rows + rr;
    cur = C.W[0][idx];
    step = F::zero();
    if (C.J == 2) {
        const fe_t w1 = C.W[1][idx];
        if (C.half) {
            step = F::halve(F::sub(cur, w1));
            cur = F::halve(F::add(cur, w1));
        } else {
            step = w1;
        }
    }
    for (uint32_t i = 0; i < C.pt0; ++i) cur = F::add(cur, step);
}

// thread index -> (row to evaluate, whether it exists).  Under sharding thread t is the t-th row of this rank's stripes.
__device__ __forceinline__ uint32_t shard_row(const RowCtx &C, uint32_t t, bool &live) {
    if (C.shard_world <= 1) {
        live = t < C.rows;
        return live ? t : C.rows - 1;
    }
    live = t < C.local_rows;
    if (!live) t = C.local_rows ? C.local_rows - 1 : 0;
    const uint32_t row = Stripes{C.shard_rank, C.shard_world}.global_index(t);
    if (row >= C.rows) { live = false; return C.rows - 1; }
    return row;
}

// Body of a straight-line ("specialised") row-program kernel: `eval(ctx, row, pt, U)` is the compiled program.
// The point values P(0..d) are parked in LDS (thread-private column, no barrier) and the inverse Vandermonde is
// applied after the last point: keeping the d accumulators T_k live across the straight-line program cost 48 VGPRs
// and pushed the kernel into scratch spills at 2 waves/SIMD.
template <class F, class Eval>
__device__ __forceinline__ void spec_kernel_body(const DevArgs &A, Eval eval) {
    __shared__ fe_t Pv[(DMAX + 1) * RP_THREADS];
    bool live;
    const uint32_t row = shard_row(A.ctx, blockIdx.x * RP_THREADS + threadIdx.x, live);
    for (uint32_t pt = 0; pt < A.npts; ++pt) {
        fe_t P = eval(A.ctx, row, pt, A.utab + (size_t)pt * A.n_uniform);
        if (A.d == 0) {
            if (live) A.out[0][row] = P;
        } else {
            Pv[pt * RP_THREADS + threadIdx.x] = P;
        }
    }
    if (A.d && live) {
        for (uint32_t k = 0; k < A.d; ++k) {
            fe_t T = F::zero();
            for (uint32_t pt = 0; pt < A.npts; ++pt) T = F::add(T, F::mul(A.vinv[k * A.npts + pt], Pv[pt * RP_THREADS + threadIdx.x]));
            A.out[k][row] = T;
        }
    }
}

// ---- sweep form: per-point accumulators of a thread in LDS, limb-planar: word `limb` of point `pt` lives at
// acc[(pt * 9 + limb) * RP_THREADS] (acc already offset by the thread index): conflict-free 4-byte lanes.  The values are LAZY
// 9 x 29-bit sums (ABI form, i.e. value * 2^256, plus a few multiples of p); sw_fold brings one below 2p again (product with
// 2^261 mod p, the radix' one), sw_finish turns it into the canonical 8 x 32 element.
constexpr uint32_t SW_WORDS = 9;
// The accumulators are DYNAMIC shared memory, sized by the launch for the points actually evaluated (sweep_smem_bytes): at
// 9 points they are 41.5 KB and only three workgroups fit a CU; the cross terms of the benchmark circuits have 6 - 7.
SRS_HD constexpr uint32_t sweep_smem_bytes(uint32_t npts) { return npts * SW_WORDS * RP_THREADS * 4u; }
__device__ __forceinline__ f29_t sw_load(const uint32_t *acc, uint32_t pt) {
    f29_t o;
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) o.v[i] = acc[(pt * SW_WORDS + i) * RP_THREADS];
    SRS_F29_LDS_LOAD(o, acc + pt * SW_WORDS * RP_THREADS);
    return o;
}
__device__ __forceinline__ void sw_store(uint32_t *acc, uint32_t pt, const f29_t &x) {
#pragma unroll
    for (uint32_t i = 0; i < 9; ++i) acc[(pt * SW_WORDS + i) * RP_THREADS] = x.v[i];
    SRS_F29_LDS_STORE(acc + pt * SW_WORDS * RP_THREADS, x);
}
template <class F>
__device__ __forceinline__ void sw_fold(uint32_t *acc, uint32_t pt, const fe_t &one261) {
    using G = Fp29<typename F::Params>;
    sw_store(acc, pt, G::mul(sw_load(acc, pt), G::unpack(one261)));
}
template <class F>
__device__ __forceinline__ fe_t sw_finish(const uint32_t *acc, uint32_t pt, const fe_t &one261) {
    using G = Fp29<typename F::Params>;
    return G::to_canonical_fe(G::mul(sw_load(acc, pt), G::unpack(one261)));
}

// The kernel body for a program in sweep form: `sweep(ctx, row, npts, utab, nu, acc, accumulate)`, `one_idx` = index of 2^261 mod p
// in the uniform table.  The inverse Vandermonde step runs on the 9 x 29-bit multiplier as well: vinv29 = vinv * 2^5, so the
// product of an ABI-form point value with it is ABI form again; the d sums are reduced once each.
template <class F, class Sweep>
__device__ __forceinline__ void sweep_kernel_body(const DevArgs &A, uint32_t one_idx, Sweep sweep) {
    using G = Fp29<typename F::Params>;
    SRS_SWEEP_ACC(acc_all);
    uint32_t *acc = acc_all + threadIdx.x;
    bool live;
    const uint32_t row = shard_row(A.ctx, blockIdx.x * RP_THREADS + threadIdx.x, live);
    sweep(A.ctx, row, A.npts, A.utab, A.n_uniform, acc, false);
    if (!live) return;
    const fe_t one261 = A.utab[one_idx];
    if (A.d == 0) {
        A.out[0][row] = sw_finish<F>(acc, 0, one261);
        return;
    }
    for (uint32_t pt = 0; pt < A.npts; ++pt) sw_fold<F>(acc, pt, one261);          // < 2p: d products each below
    for (uint32_t k = 0; k < A.d; ++k) {
        f29_t T = G::mul(sw_load(acc, 0), G::unpack(A.vinv29[k * A.npts]));
        for (uint32_t pt = 1; pt < A.npts; ++pt)
            T = G::normalize(G::add_lazy(T, G::mul(sw_load(acc, pt), G::unpack(A.vinv29[k * A.npts + pt]))));   // <= 2 (d + 1) p <= 18 p
        A.out[k][row] = G::to_canonical_fe(G::mul(T, G::unpack(one261)));
    }
}

// ---------------------------------------------------------------------------------------------
// ProtoGalaxy leaves (rowprog.hip: "ProtoGalaxy: pow-weighted sums of gate evaluations").  The argument blocks and the kernel bodies
// live here so that the ahead-of-time kernels (rowprog.hip, gate-set functor PgSpecCall<F, ID> of rowprog_spec.inc) and the kernels
// compiled at run time for any other gate set (pg_leaf_unit_source) are the SAME code.  A gate-set functor PC has
//   PC::run(gate, C, row, pt, U) -> fe_t          the straight-line program of `gate` at one point
//   PC::sweep(gate, C, row, npts, U, nu, acc, accumulate)      its sweep form, all points per column load
//   PC::one(gate)                                 index of 2^261 mod p in that gate's uniform table
// ---------------------------------------------------------------------------------------------
struct GateProg {
    const Insn *prog;
    uint32_t n_insn, result, n_uniform, utab_off;   // utab_off: offset (in fe) of this gate's table in PgArgs.utab
};
struct PgArgs {
    const GateProg *gates;
    uint32_t n_gates, log_rows;
    RowCtx ctx;
    int compat;               // Q1: row_index = index & 2^k  ==> every leaf is evaluated at row 0
    uint32_t leaf_pts;        // 1 (F, e) or P (G)
    uint32_t P;
    const fe_t *utab;         // per gate: [leaf_pts][n_uniform]
    const fe_t *weights;      // [levels][wpts]
    uint32_t wpts;            // P (F) or 1 (G, e)
    uint32_t tile_log;        // leaves per workgroup = 2^tile_log (<= 7)
    fe_t *partial;            // [n_gates * tiles_per_gate][P]
    uint32_t shard_rank, shard_world;   // process-per-GPU runs (set_shard): a 1024-leaf tile IS a key stripe (STRIPE_LOG), this rank
                              //   evaluates the tiles t % world == rank and leaves zeros for the others: its result is a PARTIAL sum
    // reference leaf rows (compat): every leaf of a gate is that gate AT ROW 0 -- one value per (gate, point) for the whole launch.  r03 shared it
    // among the 8 leaves of a thread; r04 hoists it out of the leaf pass: a one-workgroup launch (hoist_mode 1) evaluates the gates and leaves
    // hoist[gate * P + p], the leaf launch (hoist_mode 2) reads it -- every leaf still enters the tree with its own weight.  0: evaluate per thread.
    fe_t *hoist;
    int hoist_mode;
};
__device__ __forceinline__ bool pg_tile_is_mine(const PgArgs &A, uint32_t tile) {
    return A.shard_world <= 1 || tile % A.shard_world == A.shard_rank;
}
// a tile of another rank: zero partial sums (block-uniform exit before any barrier)
template <class F>
__device__ __forceinline__ void pg_zero_partial(const PgArgs &A, uint32_t gate, uint32_t tile) {
    for (uint32_t p = threadIdx.x; p < A.P; p += blockDim.x) A.partial[((size_t)gate * gridDim.x + tile) * A.P + p] = F::zero();
}

// binary-tree combine of blockDim.x values: v[2t] + v[2t+1] * w[level]; result in red[0]
template <class F>
__device__ __forceinline__ void weighted_tree(fe_t *red, fe_t x, const fe_t *__restrict__ w, uint32_t wstride, uint32_t levels) {
    const uint32_t tid = threadIdx.x;
    red[tid] = x;
    __syncthreads();
    for (uint32_t l = 0; l < levels; ++l) {
        uint32_t stride = 1u << l;
        if ((tid & (2 * stride - 1)) == 0) red[tid] = F::add(red[tid], F::mul(red[tid + stride], w[(size_t)l * wstride]));
        __syncthreads();
    }
}

SRS_HD constexpr uint32_t pg_lpt_log(uint32_t lpt) { return lpt == 8 ? 3 : (lpt == 4 ? 2 : (lpt == 2 ? 1 : 0)); }

// Body of k_pg_leaves_spec: the leaf mapping and tree of k_pg_leaves (rowprog.hip) with the gate programs as straight-line code:
// no LDS register file, no decode.  `red`: RP_THREADS elements of LDS.
template <class F, class PC, uint32_t LPT>
__device__ __forceinline__ void pg_leaves_spec_body(const PgArgs &A, fe_t *red) {
    constexpr uint32_t LPT_LOG = pg_lpt_log(LPT);
    const uint32_t gate = blockIdx.y, tile = blockIdx.x;
    if (!pg_tile_is_mine(A, tile)) { pg_zero_partial<F>(A, gate, tile); return; }
    const GateProg G = A.gates[gate];
    const uint32_t TL = A.tile_log - LPT_LOG;
    const uint32_t row0 = (tile << A.tile_log) + threadIdx.x;
    fe_t v[LPT];
    for (uint32_t p = 0; p < A.P; ++p) {
        if (A.leaf_pts > 1 || p == 0) {
#pragma unroll
            for (uint32_t l = 0; l < LPT; ++l)
                v[l] = PC::run(gate, A.ctx, A.compat ? 0u : row0 + (l << TL), p, A.utab + G.utab_off + (size_t)p * G.n_uniform);
        }
        const fe_t *w = A.weights + (A.wpts > 1 ? p : 0);
        fe_t t[LPT];
#pragma unroll
        for (uint32_t l = 0; l < LPT; ++l) t[l] = v[l];
#pragma unroll
        for (uint32_t lvl = 0; lvl < LPT_LOG; ++lvl) {
            fe_t c = w[(size_t)(TL + lvl) * A.wpts];
#pragma unroll
            for (uint32_t i = 0; i < (LPT >> (lvl + 1)); ++i) t[i] = F::add(t[2 * i], F::mul(t[2 * i + 1], c));
        }
        weighted_tree<F>(red, t[0], w, A.wpts, TL);
        if (threadIdx.x == 0) A.partial[((size_t)gate * gridDim.x + tile) * A.P + p] = red[0];
        __syncthreads();
    }
}

// Body of k_pg_leaves_sweep, the sweep form (compute_G with integer points, evaluate_e): every leaf row is swept ONCE for all P points
// (its columns are read once, the Lagrange fold advances by one addition per point).  The thread's LPT leaves need the weights
// w_l = prod_{b in bits(l)} c_(TL + b) of the leaf-index bits it owns: the host multiplies the term coefficients of the
// uniform table by w_l (one table per l, A.utab = [gate][l][P][nu]), so leaf l simply ACCUMULATES onto the same lazy 9 x 29-bit
// sums in LDS; between leaves the sums are folded below 2p.  Needs wpts == 1, P <= DMAX + 1 and affine advice leaves.
// `red`: RP_THREADS elements of LDS; `acc_all`: sweep_smem_bytes(P) of (dynamic) LDS.
template <class F, class PC, uint32_t LPT, bool COMPAT>
__device__ __forceinline__ void pg_leaves_sweep_body(const PgArgs &A, fe_t *red, uint32_t *acc_all) {
    constexpr uint32_t LPT_LOG = pg_lpt_log(LPT);
    const uint32_t gate = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
    if (!(COMPAT && A.hoist_mode == 1) && !pg_tile_is_mine(A, tile)) { pg_zero_partial<F>(A, gate, tile); return; }
    const GateProg G = A.gates[gate];
    const uint32_t TL = A.tile_log - LPT_LOG;
    const uint32_t row0 = (tile << A.tile_log) + tid;
    uint32_t *acc = acc_all + tid;
    const fe_t *U0 = A.utab + G.utab_off;
    const fe_t one261 = U0[PC::one(gate)];
    if constexpr (COMPAT) {
        // the reference's leaf rows (`index & 2^k`, src/plonk/mod.rs:714): the LPT leaves of a thread all sit at row 0 of this gate,
        // so they share ONE gate evaluation f(X_p); sum_l w_l f = (sum_l w_l) f exactly -- table LPT holds the term coefficients
        // times the sum of the thread's leaf weights (pg_sum).  The value is the same for every thread of every tile: hoisted (PgArgs::hoist)
        if (A.hoist_mode == 2) {                                // the leaf launch: the hoisted values, then the trees
            for (uint32_t p = 0; p < A.P; ++p) {
                weighted_tree<F>(red, A.hoist[(size_t)gate * A.P + p], A.weights, A.wpts, TL);
                if (tid == 0) A.partial[((size_t)gate * gridDim.x + tile) * A.P + p] = red[0];
                __syncthreads();
            }
            return;
        }
        if (A.hoist_mode == 1) {                                // the hoisting launch, grid = (P, gates): workgroup p evaluates point p alone
            RowCtx c = A.ctx;                                   // (the points are independent: P short chains side by side instead of one long one)
            c.pt0 += tile;
            PC::sweep(gate, c, 0u, 1u, U0 + ((size_t)LPT * A.P + tile) * G.n_uniform, G.n_uniform, acc, false);
            if (tid == 0) A.hoist[(size_t)gate * A.P + tile] = sw_finish<F>(acc, 0, one261);
            return;
        }
        PC::sweep(gate, A.ctx, 0u, A.P, U0 + (size_t)LPT * A.P * G.n_uniform, G.n_uniform, acc, false);
    } else {
        for (uint32_t l = 0; l < LPT; ++l) {
            PC::sweep(gate, A.ctx, row0 + (l << TL), A.P, U0 + (size_t)l * A.P * G.n_uniform, G.n_uniform, acc, l != 0);
            if (l + 1 < LPT)
                for (uint32_t p = 0; p < A.P; ++p) sw_fold<F>(acc, p, one261);
        }
    }
    for (uint32_t p = 0; p < A.P; ++p) {
        weighted_tree<F>(red, sw_finish<F>(acc, p, one261), A.weights, A.wpts, TL);
        if (tid == 0) A.partial[((size_t)gate * gridDim.x + tile) * A.P + p] = red[0];
        __syncthreads();
    }
}

// compute_F as a POLYNOMIAL tree (rowprog.hip, k_pg_F_leaves): the weights of the three leaf-index bits a thread folds, and the
// argument block of the run-time compiled kernel (one struct by value: jit::launch)
struct PgFLevels {
    fe_t beta[3], delta[3];      // weights of leaf-index bits TL, TL + 1, TL + 2
};
struct PgFArgs {
    PgArgs A;
    PgFLevels Lv;
    fe_t *nodes;
    uint32_t n_nodes;
};
// one leaf of F through a gate-set functor: the sweep form with one point (the 9 x 29-bit multiplier; `acc`: SW_WORDS words per thread
// of LDS, limb-planar, already offset by the thread index), or the straight-line program
template <class F, class PC>
struct PgFLeafSweep {
    uint32_t *acc;
    __device__ __forceinline__ fe_t operator()(const PgArgs &A, const GateProg &G, uint32_t gate, uint32_t row) const {
        PC::sweep(gate, A.ctx, row, 1, A.utab + G.utab_off, G.n_uniform, acc, false);
        return sw_finish<F>(acc, 0, (A.utab + G.utab_off)[PC::one(gate)]);
    }
};
template <class F, class PC>
struct PgFLeafRun {
    __device__ __forceinline__ fe_t operator()(const PgArgs &A, const GateProg &G, uint32_t gate, uint32_t row) const {
        return PC::run(gate, A.ctx, row, 0, A.utab + G.utab_off);
    }
};
// Body of k_pg_F_leaves: every thread evaluates its 8 leaves (`leaf(A, G, gate, row)`; same coalesced mapping as the leaf kernels above)
// and folds them over the three leaf-index bits it owns into a cubic; nodes are stored coefficient-major nodes[m * n_nodes + node].
template <class F, class Leaf>
__device__ __forceinline__ void pg_F_leaves_body(const PgArgs &A, const PgFLevels &Lv, fe_t *__restrict__ nodes, uint32_t n_nodes, Leaf leaf) {
    constexpr uint32_t LPT = 8, LPT_LOG = 3;
    const uint32_t gate = blockIdx.y, tile = blockIdx.x;
    if (!(A.compat && A.hoist_mode == 1) && !pg_tile_is_mine(A, tile)) {          // another rank's tile: zero cubic
        const uint32_t node = (gate * gridDim.x + tile) * blockDim.x + threadIdx.x;
        for (uint32_t m = 0; m < 4; ++m) nodes[(size_t)m * n_nodes + node] = F::zero();
        return;
    }
    const GateProg G = A.gates[gate];
    const uint32_t TL = A.tile_log - LPT_LOG;
    const uint32_t row0 = (tile << A.tile_log) + threadIdx.x;
    fe_t v[LPT];
#pragma unroll
    for (uint32_t l = 0; l < LPT; ++l) {
        if (A.compat && l) {                               // reference leaf rows (src/plonk/mod.rs:714): all LPT leaves are the gate at row 0
            v[l] = v[0];
            continue;
        }
        if (A.compat && A.hoist_mode == 2) {               // ... evaluated once per launch (PgArgs::hoist)
            v[0] = A.hoist[gate];
            continue;
        }
        v[l] = leaf(A, G, gate, A.compat ? 0u : row0 + (l << TL));
        if (A.compat && A.hoist_mode == 1) {               // the one-workgroup launch: the gate at row 0, nothing else
            if (threadIdx.x == 0) A.hoist[gate] = v[0];
            return;
        }
    }
    fe_t c0[4], c1[4];                                     // bit TL: (v0 + v1 (beta + X delta))
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        c0[j] = F::add(v[2 * j], F::mul(v[2 * j + 1], Lv.beta[0]));
        c1[j] = F::mul(v[2 * j + 1], Lv.delta[0]);
    }
    fe_t e0[2], e1[2], e2[2];                              // bit TL + 1
#pragma unroll
    for (uint32_t j = 0; j < 2; ++j) {
        e0[j] = F::add(c0[2 * j], F::mul(c0[2 * j + 1], Lv.beta[1]));
        e1[j] = F::add(F::add(c1[2 * j], F::mul(c1[2 * j + 1], Lv.beta[1])), F::mul(c0[2 * j + 1], Lv.delta[1]));
        e2[j] = F::mul(c1[2 * j + 1], Lv.delta[1]);
    }
    const uint32_t node = (gate * gridDim.x + tile) * blockDim.x + threadIdx.x;      // bit TL + 2
    nodes[(size_t)0 * n_nodes + node] = F::add(e0[0], F::mul(e0[1], Lv.beta[2]));
    nodes[(size_t)1 * n_nodes + node] = F::add(F::add(e1[0], F::mul(e1[1], Lv.beta[2])), F::mul(e0[1], Lv.delta[2]));
    nodes[(size_t)2 * n_nodes + node] = F::add(F::add(e2[0], F::mul(e2[1], Lv.beta[2])), F::mul(e1[1], Lv.delta[2]));
    nodes[(size_t)3 * n_nodes + node] = F::mul(e2[1], Lv.delta[2]);
}

}  // namespace rowprog
}  // namespace srs
