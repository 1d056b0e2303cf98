// rowprog.hip -- per-row polynomial work of the Sangria NIFS on gfx950:
//   * cross terms  T_k[row], k = 1..d   (reference VanillaFS::commit_cross_terms, src/nifs/sangria/mod.rs:102-158)
//   * plain gate evaluation per row       (deciders, src/nifs/sangria/mod.rs:334-383, src/plonk/mod.rs:304-361)
//   * witness / error-vector folds        (RelaxedPlonkWitness::fold, src/nifs/sangria/accumulator.rs:364-404)
//
// What the reference computes: with P the compressed + homogenised gate polynomial of the structure
// (src/plonk/util.rs:34-56, src/polynomial/expression.rs:356-429, src/plonk/mod.rs:68-121),
//   T_k[row] = coefficient of X^k in  P(fixed[row], W1[row] + X*W2[row], ch1 + X*ch2)
// obtained symbolically (GroupedPoly::new, src/polynomial/grouped_poly.rs:88-138) and evaluated by a
// per-row interpreter, one pass over all columns PER TERM (src/polynomial/graph_evaluator.rs:361-388).
//
// MI355X-first formulation: the coefficients are mathematically determined, and field arithmetic
// is exact, so they are recovered numerically instead -- evaluate P at the d+1 points X = 0..d and
// apply the (constant) inverse Vandermonde matrix.  One pass over the rows yields ALL d terms.
// This file holds the kernels and their launch code; the programs they run (SSA register programs, the
// host-evaluated "uniform table", the emitted straight-line and sweep sources) come from the host-only
// compiler in rowprog_compile.hip.
// Row registers live in LDS as [slot][thread] (conflict-free 32-byte lanes); the d accumulators
// T_k live in VGPRs.  Columns are read coalesced (column-major, consecutive rows per lane).
#include "rowprog.h"
#include "rowprog_compile.h"
#include "ntt.h"
#include "prof.h"
#include "jit.h"
#include "tuning.h"

#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

namespace srs {
namespace rowprog {

// device-side definitions (RowCtx, DevArgs, column loads, specialised-kernel body): rowprog_dev.cuh
// interpret one row program at evaluation point `pt`; registers = LDS slots [slot][thread]
template <class F>
__device__ __forceinline__ fe_t interp(fe_t *slots, const Insn *__restrict__ prog, uint32_t n_insn, uint32_t result,
                                       const RowCtx &C, uint32_t row, uint32_t pt, const fe_t *__restrict__ U) {
    const uint32_t tid = threadIdx.x, nthr = blockDim.x, mask = C.rows - 1;
    for (uint32_t ip = 0; ip < n_insn; ++ip) {
        const Insn in = prog[ip];
        fe_t r;
        if (in.op <= I_LD_ADV) {
            uint32_t rr = (row + (uint32_t)(int32_t)in.b) & mask;     // (row + rot) rem_euclid 2^k
            if (in.op == I_LD_SEL) r = ld_sel<F>(C, in.a, rr);
            else if (in.op == I_LD_FIX) r = ld_fix<F>(C, in.a, rr);
            else r = ld_adv<F>(C, in.a, rr, pt);
        } else {
            fe_t a = (in.a & UNIFORM_BIT) ? U[in.a & ~UNIFORM_BIT] : slots[in.a * nthr + tid];
            if (in.op <= I_MUL) {
                fe_t b = (in.b & UNIFORM_BIT) ? U[in.b & ~UNIFORM_BIT] : slots[in.b * nthr + tid];
                r = in.op == I_ADD ? F::add(a, b) : (in.op == I_SUB ? F::sub(a, b) : F::mul(a, b));
            } else if (in.op == I_SQR) {
                r = F::sqr(a);
            } else if (in.op == I_DBL) {
                r = F::dbl(a);
            } else {
                r = F::neg(a);
            }
        }
        slots[in.dst * nthr + tid] = r;
    }
    return (result & UNIFORM_BIT) ? U[result & ~UNIFORM_BIT] : slots[result * nthr + tid];
}

template <class F, uint32_t NSLOT>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 1) k_rowprog(DevArgs A) {
    __shared__ fe_t slots[NSLOT * RP_THREADS];
    bool live;
    const uint32_t row = shard_row(A.ctx, blockIdx.x * RP_THREADS + threadIdx.x, live);
    fe_t T[DMAX];
#pragma unroll
    for (uint32_t k = 0; k < DMAX; ++k) T[k] = F::zero();
    for (uint32_t pt = 0; pt < A.npts; ++pt) {
        fe_t P = interp<F>(slots, A.prog, A.n_insn, A.result, A.ctx, row, pt, A.utab + (size_t)pt * A.n_uniform);
        if (A.d == 0) {
            if (live) A.out[0][row] = P;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < DMAX; ++k) {
                if (k < A.d) T[k] = F::add(T[k], F::mul(A.vinv[k * A.npts + pt], P));
            }
        }
    }
    if (A.d && live) {
#pragma unroll
        for (uint32_t k = 0; k < DMAX; ++k)
            if (k < A.d) A.out[k][row] = T[k];
    }
}

// ---------------------------------------------------------------------------------------------
// Specialised row programs.  The interpreter above is the general path (any circuit).  For the gate
// sets of the reference's own configurations (MainGate<5> + MainGate<3>, MainGate<5>: SURVEY.md H5)
// the SSA program is additionally emitted as straight-line C++ (emit_spec_source, rowprog_compile.hip), compiled
// ahead of time (tools/gen_rowprog_spec.py -> rowprog_spec.inc) and selected by program
// fingerprint: registers instead of LDS slots, no decode, loads scheduled by the compiler.
// ---------------------------------------------------------------------------------------------
#define SRS_SPEC_PART 1
#include "rowprog_spec.inc"
#undef SRS_SPEC_PART

template <class F, int ID>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 2) k_rowprog_spec(DevArgs A) {
    // sweep form: every column is read once for all points, bodies on the 9 x 29-bit multiplier.  The callers of these kernels
    // (cross terms, plain gate evaluation) never pass a coefficient table, and the specialised programs have d <= DMAX.
    sweep_kernel_body<F>(A, SpecCall<F, ID>::one(), [](const RowCtx &C, uint32_t row, uint32_t npts, const fe_t *U, uint32_t nu, uint32_t *acc, bool accumulate) {
        SpecCall<F, ID>::sweep(C, row, npts, U, nu, acc, accumulate);
    });
}

// ---------------------------------------------------------------------------------------------
// ProtoGalaxy: pow-weighted sums of gate evaluations (reference src/nifs/protogalaxy/poly/mod.rs)
//   Out[p] = sum_{i < n} pow_i(c^(p)) * f_i^(p),   pow_i(c) = prod_{b in bits(i)} c_b
//   f_i = gates[i / 2^k] evaluated at row(i)  (get_evaluate_witness_fn, src/plonk/mod.rs:683-718)
// compute_F : one leaf value, P weight vectors c^(p) = beta + X_p * delta          (:68-203)
// compute_G : P leaf values (witness folded with L_j(X_p) on the fly -- FoldedWitness is never
//             materialised), one weight vector beta'                                (:308-425)
// evaluate_e: P = 1                                                   (protogalaxy/mod.rs:571-640)
// The reference reduces with a binary tree where the right child is scaled by c_height; the same
// tree is evaluated here level by level (LDS inside a workgroup, then across workgroups).
// The argument blocks (GateProg, PgArgs, PgFLevels), the tile ownership, the weighted tree and the bodies of the specialised leaf
// kernels are in rowprog_dev.cuh: the kernels compiled at run time for other gate sets (pg_leaf_unit_source) share them.
// ---------------------------------------------------------------------------------------------
// grid = (tiles_per_gate, n_gates), block = T = 2^(tile_log - log2 LPT) threads.  Thread t owns the LPT leaves
// base + l * T + t (l < LPT): consecutive lanes read consecutive rows, so every column load is coalesced.  The sum
// sum_i pow_i(c) f_i does not care about the order of additions (exact arithmetic), only that leaf i meets the weights
// of ITS index bits: the in-register combine over l therefore uses the weights of bits log2(T).., the LDS tree over
// the threads those of bits 0 .. log2(T) - 1.
template <class F, uint32_t NSLOT, uint32_t LPT>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 1) k_pg_leaves(PgArgs A) {
    __shared__ fe_t slots[NSLOT * RP_THREADS];
    __shared__ fe_t red[RP_THREADS];
    constexpr uint32_t LPT_LOG = pg_lpt_log(LPT);
    const uint32_t gate = blockIdx.y, tile = blockIdx.x;
    const GateProg G = A.gates[gate];
    if (A.compat && A.hoist_mode == 1) {      // r06, as the ahead-of-time kernels: the reference's leaf rows make every leaf of a gate that gate AT ROW 0 --
        // the hoisting launch, grid = (leaf_pts, gates), evaluates it once per (gate, point); every lane computes the same value, lane 0 stores it
        const fe_t x = interp<F>(slots, G.prog, G.n_insn, G.result, A.ctx, 0u, tile, A.utab + G.utab_off + (size_t)tile * G.n_uniform);
        if (threadIdx.x == 0) A.hoist[(size_t)gate * A.leaf_pts + tile] = x;
        return;
    }
    if (!pg_tile_is_mine(A, tile)) { pg_zero_partial<F>(A, gate, tile); return; }
    const uint32_t TL = A.tile_log - LPT_LOG;                          // log2(blockDim.x)
    const uint32_t row0 = (tile << A.tile_log) + threadIdx.x;          // < rows (rows is a multiple of the tile)
    fe_t v[LPT];
    for (uint32_t p = 0; p < A.P; ++p) {
        if (A.compat && A.hoist_mode == 2) {                           // the leaf launch reads the hoisted values
            if (A.leaf_pts > 1 || p == 0) {
                const fe_t x = A.hoist[(size_t)gate * A.leaf_pts + (A.leaf_pts > 1 ? p : 0)];
#pragma unroll
                for (uint32_t l = 0; l < LPT; ++l) v[l] = x;
            }
        } else if (A.leaf_pts > 1 || p == 0) {
#pragma unroll
            for (uint32_t l = 0; l < LPT; ++l)
                v[l] = interp<F>(slots, G.prog, G.n_insn, G.result, A.ctx, A.compat ? 0u : row0 + (l << TL), p,
                                 A.utab + G.utab_off + (size_t)p * G.n_uniform);
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

// k_pg_leaves with the gate programs of a known gate set compiled ahead of time (rowprog_spec.inc, PgSpecCall):
// no LDS register file, no decode -- same leaf mapping and tree (pg_leaves_spec_body).
template <class F, int ID, uint32_t LPT>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 2) k_pg_leaves_spec(PgArgs A) {
    __shared__ fe_t red[RP_THREADS];
    pg_leaves_spec_body<F, PgSpecCall<F, ID>, LPT>(A, red);
}

// k_pg_leaves_spec in sweep form (compute_G with integer points, evaluate_e): every leaf row is swept ONCE for all P points
// (pg_leaves_sweep_body)
template <class F, int ID, uint32_t LPT, bool COMPAT>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 2) k_pg_leaves_sweep(PgArgs A) {
    __shared__ fe_t red[RP_THREADS];
    SRS_SWEEP_ACC(acc_all);                                 // sweep_smem_bytes(P) of dynamic LDS
    pg_leaves_sweep_body<F, PgSpecCall<F, ID>, LPT, COMPAT>(A, red, acc_all);
}

// compute_F as a POLYNOMIAL tree (no evaluation points, no ifft).  F(X) = sum_i f_i prod_{b in bits(i)} (beta_b + X delta_b)
// has degree t = log2(#leaves); the reference evaluates it at next_pow2(t + 1) points (one weighted tree per point, t'n
// multiplies) and interpolates.  The same coefficients come out of ONE tree whose nodes are polynomials:
//   node = left + right * (beta_h + X delta_h)   ->   2 (deg + 1) multiplies per node, ~4 n in total instead of 32 n
// (exact arithmetic: identical coefficients, the ones above degree t are exactly zero in the reference's ifft too).
// k_pg_F_leaves: every thread evaluates its 8 leaves (same coalesced mapping as k_pg_leaves) and folds them over the
// three leaf-index bits it owns into a cubic; nodes are stored coefficient-major nodes[m * n_nodes + node].
template <class F, uint32_t NSLOT, int ID>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 1) k_pg_F_leaves(PgArgs A, PgFLevels Lv, fe_t *__restrict__ nodes, uint32_t n_nodes) {
    __shared__ fe_t slots[NSLOT * RP_THREADS];
    if constexpr (ID >= 0) {                               // the ahead-of-time gate set: sweep form with one point (NSLOT >= 2: 9 words per thread fit)
        pg_F_leaves_body<F>(A, Lv, nodes, n_nodes, PgFLeafSweep<F, PgSpecCall<F, (ID >= 0 ? ID : 0)>>{reinterpret_cast<uint32_t *>(slots) + threadIdx.x});
    } else {
        pg_F_leaves_body<F>(A, Lv, nodes, n_nodes, [&](const PgArgs &a, const GateProg &G, uint32_t, uint32_t row) {
            return interp<F>(slots, G.prog, G.n_insn, G.result, a.ctx, row, 0, a.utab + G.utab_off);
        });
    }
}

// one level of the polynomial tree: out[i] = in[2i] + in[2i+1] * (beta + X delta); nodes >= m_valid are zero.
// coefficient-major arrays: in[m * n_in + node] (degree deg_in), out[m * n_out + node] (degree deg_in + 1).
// One thread per (coefficient m, node i) -- consecutive threads = consecutive nodes of one coefficient (coalesced): the upper levels
// have few nodes, and a thread per NODE walking its deg + 2 coefficients in turn left them at 16-48 us of pure latency each (r02:
// 18 launches = 0.5 ms of a step); r03.
template <class F>
__global__ void k_pg_F_level(const fe_t *__restrict__ in, uint32_t n_in, uint32_t m_valid, uint32_t deg_in, fe_t beta, fe_t delta,
                             fe_t *__restrict__ out, uint32_t n_out) {
    const uint32_t lin = blockIdx.x * blockDim.x + threadIdx.x;
    if (lin >= n_out * (deg_in + 2)) return;
    const uint32_t m = lin / n_out, i = lin - m * n_out;
    const bool hasL = 2 * i < m_valid, hasR = 2 * i + 1 < m_valid;
    fe_t acc = F::zero();
    if (m <= deg_in) {
        if (hasL) acc = in[(size_t)m * n_in + 2 * i];
        if (hasR) acc = F::add(acc, F::mul(in[(size_t)m * n_in + 2 * i + 1], beta));
    }
    if (m >= 1 && hasR) acc = F::add(acc, F::mul(in[(size_t)(m - 1) * n_in + 2 * i + 1], delta));
    out[(size_t)m * n_out + i] = acc;
}

// the top of the tree in ONE workgroup: the last `nlev` <= PG_F_TAIL_LEVELS levels (n_in = 2^nlev <= 32 nodes) through LDS, the same
// (coefficient, node) threads; writes the final polynomial (degree deg_in + nlev) to out[0 .. deg_in + nlev]
constexpr uint32_t PG_F_TAIL_LEVELS = 5, PG_F_TAIL_MAXDEG = 40;
struct PgFTail {
    fe_t beta[PG_F_TAIL_LEVELS], delta[PG_F_TAIL_LEVELS];
};
template <class F>
__global__ void SRS_KERNEL_BOUNDS(512, 1)
    k_pg_F_tail(const fe_t *__restrict__ in, uint32_t n_in, uint32_t m_valid, uint32_t deg_in, uint32_t nlev, PgFTail T, fe_t *__restrict__ out) {
    __shared__ fe_t buf[2][(PG_F_TAIL_MAXDEG + 1) * 16];        // level outputs: <= 16 nodes x <= 41 coefficients
    const uint32_t t = threadIdx.x;
    uint32_t cur_n = n_in, deg = deg_in, valid = m_valid;
    for (uint32_t lv = 0; lv < nlev; ++lv) {
        const uint32_t n_out = cur_n >> 1;
        const fe_t *src = lv == 0 ? in : buf[(lv - 1) & 1];
        fe_t *dst = buf[lv & 1];
        for (uint32_t lin = t; lin < n_out * (deg + 2); lin += blockDim.x) {
            const uint32_t m = lin / n_out, i = lin - m * n_out;
            const bool hasL = 2 * i < valid, hasR = 2 * i + 1 < valid;
            fe_t acc = F::zero();
            if (m <= deg) {
                if (hasL) acc = src[(size_t)m * cur_n + 2 * i];
                if (hasR) acc = F::add(acc, F::mul(src[(size_t)m * cur_n + 2 * i + 1], T.beta[lv]));
            }
            if (m >= 1 && hasR) acc = F::add(acc, F::mul(src[(size_t)(m - 1) * cur_n + 2 * i + 1], T.delta[lv]));
            dst[(size_t)m * n_out + i] = acc;
        }
        __syncthreads();
        cur_n = n_out;
        ++deg;
        valid = (valid + 1) >> 1;
    }
    for (uint32_t m = t; m <= deg; m += blockDim.x) out[m] = buf[(nlev - 1) & 1][m];
}

// r05: SEVERAL levels of the polynomial tree per launch, for ANY number of nodes: workgroup g takes the 2^nlev consecutive input nodes
// [g 2^nlev, (g + 1) 2^nlev) through nlev <= PG_F_MULTI_LEVELS levels in LDS (the same (coefficient, node) threads as k_pg_F_level) and writes
// ONE output node of degree deg_in + nlev.  compute_F's 18 levels above the leaf cubics (k = 20) are 3 launches instead of 13 + 1
// (each ~7 us of kernel + a launch gap on a chain nothing overlaps).   grid = n_in >> nlev, block = 256
constexpr uint32_t PG_F_MULTI_LEVELS = 6, PG_F_MULTI_NODES = 1u << (PG_F_MULTI_LEVELS - 1);
struct PgFMulti {
    fe_t beta[PG_F_MULTI_LEVELS], delta[PG_F_MULTI_LEVELS];
};
template <class F>
__global__ void SRS_KERNEL_BOUNDS(256, 1)
    k_pg_F_multi(const fe_t *__restrict__ in, uint32_t n_in, uint32_t m_valid, uint32_t deg_in, uint32_t nlev, PgFMulti T, fe_t *__restrict__ out,
                 uint32_t n_out_total) {
    // level outputs, two buffers of 32 x (deg_in + nlev + 1) elements each: DYNAMIC LDS sized by the launch -- the first launch of a k = 20
    // compute_F (4096 workgroups, degree 3 -> 9) needs 20 KB and shares a CU eight ways; with the worst-case 84 KB it ran one workgroup per
    // CU, 16 rounds: 219 us (profiles/r05_ab_misc.txt)
    SRS_DYN_LDS(fe_t, dyn, 2 * (PG_F_TAIL_MAXDEG + 1) * PG_F_MULTI_NODES);
    const uint32_t bstride = PG_F_MULTI_NODES * (deg_in + nlev + 1);
    fe_t *const buf[2] = {dyn, dyn + bstride};
    const uint32_t t = threadIdx.x, g = blockIdx.x;
    const uint32_t first = g << nlev;                                      // this workgroup's first input node
    uint32_t cur_n = 1u << nlev, deg = deg_in;
    uint32_t valid = m_valid > first ? m_valid - first : 0u;               // its input nodes that are not padding
    if (valid > cur_n) valid = cur_n;
    for (uint32_t lv = 0; lv < nlev; ++lv) {
        const uint32_t n_out = cur_n >> 1;
        const fe_t *src = lv == 0 ? in + first : buf[(lv - 1) & 1];
        const size_t src_stride = lv == 0 ? (size_t)n_in : (size_t)cur_n;  // coefficient-major: src[m * stride + node]
        fe_t *dst = buf[lv & 1];
        for (uint32_t lin = t; lin < n_out * (deg + 2); lin += blockDim.x) {
            const uint32_t m = lin / n_out, i = lin - m * n_out;
            const bool hasL = 2 * i < valid, hasR = 2 * i + 1 < valid;
            fe_t acc = F::zero();
            if (m <= deg) {
                if (hasL) acc = src[(size_t)m * src_stride + 2 * i];
                if (hasR) acc = F::add(acc, F::mul(src[(size_t)m * src_stride + 2 * i + 1], T.beta[lv]));
            }
            if (m >= 1 && hasR) acc = F::add(acc, F::mul(src[(size_t)(m - 1) * src_stride + 2 * i + 1], T.delta[lv]));
            dst[(size_t)m * n_out + i] = acc;
        }
        __syncthreads();
        cur_n = n_out;
        ++deg;
        valid = (valid + 1) >> 1;
    }
    for (uint32_t m = t; m <= deg; m += blockDim.x) out[(size_t)m * n_out_total + g] = buf[(nlev - 1) & 1][m];
}

#define SRS_SPEC_PART 2
#include "rowprog_spec.inc"
#undef SRS_SPEC_PART

// continues the tree over the per-tile partials: in[m_valid][P] (zero beyond m_valid) -> out[ceil(m / 2^lv)][P]
// grid = number of output nodes, block = 2^lv threads
template <class F>
__global__ void SRS_KERNEL_BOUNDS(RP_THREADS, 1)
    k_pg_reduce(const fe_t *__restrict__ in, uint32_t m_valid, uint32_t P, const fe_t *__restrict__ weights, uint32_t wpts,
                uint32_t level0, uint32_t lv, fe_t *__restrict__ out) {
    __shared__ fe_t red[RP_THREADS];
    const uint32_t node = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t p = 0; p < P; ++p) {
        fe_t x = node < m_valid ? in[(size_t)node * P + p] : F::zero();
        weighted_tree<F>(red, x, weights + (size_t)level0 * wpts + (wpts > 1 ? p : 0), wpts, lv);
        if (threadIdx.x == 0) out[(size_t)blockIdx.x * P + p] = red[0];
        __syncthreads();
    }
}

// r05: the same reduction with the P evaluation points SIDE BY SIDE: thread (p, t) of a workgroup of P * 2^lv <= 1024 threads runs point p's
// tree (k_pg_reduce walks the points one after the other: P x lv dependent multiply-add-barrier rounds on a chain nothing overlaps --
// 64 + 26 us per compute_G at P = 5).   grid = number of output nodes, block = (2^lv, P)
constexpr uint32_t PG_REDUCE_PAR_THREADS = 1024;
template <class F>
__global__ void SRS_KERNEL_BOUNDS(PG_REDUCE_PAR_THREADS, 1)
    k_pg_reduce_par(const fe_t *__restrict__ in, uint32_t m_valid, uint32_t P, const fe_t *__restrict__ weights, uint32_t wpts,
                    uint32_t level0, uint32_t lv, fe_t *__restrict__ out) {
    __shared__ fe_t red[PG_REDUCE_PAR_THREADS];
    const uint32_t t = threadIdx.x, p = threadIdx.y, width = blockDim.x;
    const uint32_t node = blockIdx.x * width + t;
    fe_t *r = red + (size_t)p * width;
    const fe_t *w = weights + (size_t)level0 * wpts + (wpts > 1 ? p : 0);
    r[t] = node < m_valid ? in[(size_t)node * P + p] : F::zero();
    __syncthreads();
    for (uint32_t l = 0; l < lv; ++l) {
        const uint32_t stride = 1u << l;
        if ((t & (2 * stride - 1)) == 0) r[t] = F::add(r[t], F::mul(r[t + stride], w[(size_t)l * wpts]));
        __syncthreads();
    }
    if (t == 0) out[(size_t)blockIdx.x * P + p] = r[0];
}

// K(X) on the coset (compute_K_from_G, poly/mod.rs:475-509): thread i: X = ZETA * w^i,
//   K(X) = (G(X) - F(alpha) * L0(X)) / Z(X),  L0(X) = (1/n)(X^n - 1)/(X - 1),  Z(X) = X^n - 1,  n = instances_to_fold
__global__ void k_pg_K_points(const fe_t *__restrict__ polyG, uint32_t nG, fe_t f_alpha, fe_t zeta, fe_t omega, fe_t inv_n,
                              uint32_t n_fold, uint32_t count, fe_t *__restrict__ out, int *__restrict__ err) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    fe_t X = Fr::mul(zeta, Fr::pow_u64(omega, i));
    fe_t g = Fr::zero(), xp = Fr::one();
    for (uint32_t k = 0; k < nG; ++k) {            // UnivariatePoly::eval (univariate.rs:67-75)
        g = Fr::add(g, Fr::mul(xp, polyG[k]));
        xp = Fr::mul(xp, X);
    }
    fe_t xn1 = Fr::sub(Fr::pow_u64(X, n_fold), Fr::one());
    fe_t xm1 = Fr::sub(X, Fr::one());
    fe_t l0;
    if (Fr::is_zero(xn1) && Fr::is_zero(xm1)) l0 = Fr::one();   // lagrange.rs:67-69
    else l0 = Fr::mul(inv_n, Fr::mul(xn1, Fr::inv(xm1)));
    if (Fr::is_zero(xn1)) { *err = 1; return; }                 // "Z(X) must be not equal to 0"
    out[i] = Fr::mul(Fr::sub(g, Fr::mul(f_alpha, l0)), Fr::inv(xn1));
}

constexpr uint32_t PG_K_SMALL_MAX_NODES = 32, PG_K_SMALL_MAX_LOG = 12;
// r06: the same K points for a SMALL domain straight from compute_G's values at integer nodes (one incoming trace): every workgroup
// interpolates G (coefficients c = M v, M = the constant inverse Vandermonde matrix of the nodes, v = the values, v[0] = g0 when
// `has_g0`: G(1) = F(alpha)), then thread i evaluates G at X_i by Horner and applies the domain's precomputed L_0(X_i) and 1 / Z(X_i)
// (tab = [xs | l0 | inv_z], count entries each).  Exact field arithmetic: the host route's values bit for bit.
__global__ void k_pg_K_small(const fe_t *__restrict__ vals, uint32_t n_vals, fe_t g0, int has_g0, const fe_t *__restrict__ M, uint32_t n_nodes,
                             fe_t f_alpha, const fe_t *__restrict__ tab, uint32_t count, fe_t *__restrict__ out) {
    __shared__ fe_t c[PG_K_SMALL_MAX_NODES];
    if (threadIdx.x < n_nodes) {
        fe_t acc = Fr::zero();
        for (uint32_t j = 0; j < n_nodes; ++j) {
            const fe_t v = has_g0 ? (j == 0 ? g0 : vals[j - 1]) : vals[j];
            acc = Fr::add(acc, Fr::mul(M[threadIdx.x * n_nodes + j], v));
        }
        c[threadIdx.x] = acc;
    }
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const fe_t X = tab[i];
    fe_t g = Fr::zero();
    for (uint32_t k = n_nodes; k-- > 0;) g = Fr::add(Fr::mul(g, X), c[k]);
    out[i] = Fr::mul(Fr::sub(g, Fr::mul(f_alpha, tab[count + i])), tab[2 * count + i]);
}

// number of rows with a[i] != b[i] (b == nullptr: a[i] != 0): the deciders' mismatch count
// (PlonkStructure::is_sat src/plonk/mod.rs:329-346; is_sat_accumulation src/nifs/sangria/mod.rs:352-376)
__global__ void k_count_mismatch(const fe_t *__restrict__ a, const fe_t *__restrict__ b, size_t n, uint32_t *__restrict__ count) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_t x = a[i];
    bool bad = b ? !Fr::eq(x, b[i]) : !Fr::is_zero(x);
    if (bad) atomicAdd(count, 1u);
}

// ---------------------------------------------------------------------------------------------
// lookup arguments (log-derivative), src/plonk/lookup.rs
// ---------------------------------------------------------------------------------------------
// evaluate_m (lookup.rs:275-303): m[i] = #{ j : l[j] == t[i] } for the FIRST row i holding a given table value,
// 0 for its repeats.  The reference builds a HashMap over l and walks t serially; here t is inserted into an
// open-addressing table (slot = row index of the smallest row with that value, resolved with atomicMin so the
// result does not depend on scheduling), l is counted into the slots, and every row of t reads its slot back.
// Values compare by their Montgomery limbs (a bijection of the canonical form `to_repr` the reference hashes).
// A slot holds row + 1, 0 = empty: ONE clear zeroes the rows and the counts of every table together.
// blockIdx.y = the lookup: its columns lie y * n elements, its tables y * (mask + 1) slots behind the pointers (run_sps_protocol's
// witness layout, sps_lookup_round_1); a launch for one lookup has gridDim.y = 1.
constexpr uint32_t M_EMPTY = 0u;
__device__ __forceinline__ uint32_t fe_hash(const fe_t &x) {
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        h ^= x.v[i];
        h *= 0x85EBCA6Bu;
        h ^= h >> 15;
    }
    return h;
}
__global__ void k_m_insert(const fe_t *__restrict__ t, uint32_t n, uint32_t *__restrict__ slot_row, uint32_t mask) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    t += (size_t)blockIdx.y * n;
    slot_row += (size_t)blockIdx.y * ((size_t)mask + 1);
    const fe_t key = t[i];
    uint32_t s = fe_hash(key) & mask;
    for (;;) {
        uint32_t cur = atomicCAS(&slot_row[s], M_EMPTY, i + 1);
        if (cur == M_EMPTY) return;
        if (Fr::eq(t[cur - 1], key)) { atomicMin(&slot_row[s], i + 1); return; }
        s = (s + 1) & mask;
    }
}
__global__ void k_m_count(const fe_t *__restrict__ l, uint32_t n, const fe_t *__restrict__ t, const uint32_t *__restrict__ slot_row,
                          uint32_t *__restrict__ slot_cnt, uint32_t mask) {
    uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    l += (size_t)blockIdx.y * n;
    t += (size_t)blockIdx.y * n;
    slot_row += (size_t)blockIdx.y * ((size_t)mask + 1);
    slot_cnt += (size_t)blockIdx.y * ((size_t)mask + 1);
    const fe_t key = l[j];
    uint32_t s = fe_hash(key) & mask;
    for (;;) {
        uint32_t cur = slot_row[s];
        if (cur == M_EMPTY) return;                       // value not in the table
        if (Fr::eq(t[cur - 1], key)) { atomicAdd(&slot_cnt[s], 1u); return; }
        s = (s + 1) & mask;
    }
}
template <class F>
__global__ void k_m_emit(const fe_t *__restrict__ t, uint32_t n, const uint32_t *__restrict__ slot_row,
                         const uint32_t *__restrict__ slot_cnt, uint32_t mask, fe_t *__restrict__ m) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    t += (size_t)blockIdx.y * n;
    m += (size_t)blockIdx.y * n;
    slot_row += (size_t)blockIdx.y * ((size_t)mask + 1);
    slot_cnt += (size_t)blockIdx.y * ((size_t)mask + 1);
    const fe_t key = t[i];
    uint32_t s = fe_hash(key) & mask;
    for (;;) {
        uint32_t cur = slot_row[s];
        if (cur == i + 1 || Fr::eq(t[cur - 1], key)) break;     // every row of t was inserted: the probe terminates, on a filled slot
        s = (s + 1) & mask;
    }
    uint32_t c = slot_row[s] == i + 1 ? slot_cnt[s] : 0u;
    m[i] = c ? F::from_u64(c) : F::zero();               // F::from_u128(count), lookup.rs:295-300
}

// evaluate_h_g (lookup.rs:305-317): h = 1 / (l + r), g = m / (t + r), with 1/0 := 0.
// One field inversion per HG_CHUNK elements (Montgomery's trick); elements of a chunk are blockDim apart, so
// every load / store is coalesced.  blockIdx.y: 0 -> h, 1 -> g.  blockIdx.z = the lookup: its five columns lie z * n elements behind
// the pointers (sps_lookup_round_2); a launch for one lookup has gridDim.z = 1.
constexpr uint32_t HG_THREADS = 128, HG_CHUNK = 8;
template <class F>
__global__ void SRS_KERNEL_BOUNDS(HG_THREADS, 1)
k_lookup_hg(const fe_t *__restrict__ l, const fe_t *__restrict__ t, const fe_t *__restrict__ m, fe_t r, uint32_t n,
            fe_t *__restrict__ h, fe_t *__restrict__ g) {
    const bool is_g = blockIdx.y == 1;
    const size_t col = (size_t)blockIdx.z * n;
    const fe_t *__restrict__ src = (is_g ? t : l) + col;
    fe_t *__restrict__ dst = (is_g ? g : h) + col;
    m += col;
    const uint32_t base = blockIdx.x * HG_THREADS * HG_CHUNK + threadIdx.x;
    fe_t v[HG_CHUNK], pref[HG_CHUNK];
    uint32_t zero_mask = 0;
    fe_t acc = F::one();
#pragma unroll
    for (uint32_t j = 0; j < HG_CHUNK; ++j) {
        uint32_t idx = base + j * HG_THREADS;
        fe_t x = idx < n ? F::add(src[idx], r) : F::one();
        if (F::is_zero(x)) { zero_mask |= 1u << j; x = F::one(); }
        v[j] = x;
        pref[j] = acc;
        acc = F::mul(acc, x);
    }
    fe_t inv = F::inv(acc);
#pragma unroll
    for (int j = (int)HG_CHUNK - 1; j >= 0; --j) {
        uint32_t idx = base + (uint32_t)j * HG_THREADS;
        fe_t o = F::mul(inv, pref[j]);
        inv = F::mul(inv, v[j]);
        if (idx < n) {
            if ((zero_mask >> j) & 1u) o = F::zero();
            else if (is_g) o = F::mul(o, m[idx]);
            dst[idx] = o;
        }
    }
}

// batch_invert_assigned (src/util/mod.rs:119-153): out[i] = num[i] * (has_den[i] ? den[i]^-1 : 1), with 0^-1 := 0
// (ff::BatchInvert leaves zero denominators at zero).  Same chunked Montgomery trick and access pattern as k_lookup_hg.
template <class F>
__global__ void SRS_KERNEL_BOUNDS(HG_THREADS, 1)
k_assigned_invert(const fe_t *__restrict__ num, const fe_t *__restrict__ den, const uint8_t *__restrict__ has_den, uint32_t n,
                  fe_t *__restrict__ out) {
    const uint32_t base = blockIdx.x * HG_THREADS * HG_CHUNK + threadIdx.x;
    fe_t v[HG_CHUNK], pref[HG_CHUNK];
    uint32_t zero_mask = 0, triv_mask = 0;
    fe_t acc = F::one();
#pragma unroll
    for (uint32_t j = 0; j < HG_CHUNK; ++j) {
        uint32_t idx = base + j * HG_THREADS;
        fe_t x = F::one();
        if (idx < n && (!has_den || has_den[idx])) {
            x = den[idx];
            if (F::is_zero(x)) { zero_mask |= 1u << j; x = F::one(); }
        } else {
            triv_mask |= 1u << j;
        }
        v[j] = x;
        pref[j] = acc;
        acc = F::mul(acc, x);
    }
    fe_t inv = F::inv(acc);
#pragma unroll
    for (int j = (int)HG_CHUNK - 1; j >= 0; --j) {
        uint32_t idx = base + (uint32_t)j * HG_THREADS;
        fe_t o = F::mul(inv, pref[j]);
        inv = F::mul(inv, v[j]);
        if (idx < n) {
            fe_t a = num[idx];
            if ((zero_mask >> j) & 1u) a = F::zero();
            else if (!((triv_mask >> j) & 1u)) a = F::mul(a, o);
            out[idx] = a;
        }
    }
}

// partial sums of a[i] - b[i] (is_sat_log_derivative, src/plonk/mod.rs:366-378): one value per workgroup
template <class F>
__global__ void k_sum_diff(const fe_t *__restrict__ a, const fe_t *__restrict__ b, uint32_t n, fe_t *__restrict__ partial) {
    __shared__ fe_t red[256];
    fe_t acc = F::zero();
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) acc = F::add(acc, F::sub(a[i], b[i]));
    red[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t s = blockDim.x / 2; s > 0; s >>= 1) {
        if (threadIdx.x < s) red[threadIdx.x] = F::add(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// out[i] = sum_j coef[j] * W[j][i]   (ProtoGalaxy::fold_witness, protogalaxy/mod.rs:176-210)
struct LincombArgs {
    const fe_t *w[JMAX];
    fe_t coef[JMAX];
    uint32_t J;
};
// AFFINE: the coefficients sum to one (Lagrange values, the only caller on the hot path: ProtoGalaxy::fold_witness), so
// sum_j c_j w_j = w_0 + sum_{j>=1} c_j (w_j - w_0): one product less per element, the same field element.
// world > 1 (process-per-GPU ranks): n counts the elements of THIS rank's block-cyclic stripes; only those are folded.
template <class F, bool AFFINE>
__global__ void k_lincomb(fe_t *__restrict__ out, LincombArgs a, size_t n, uint32_t rank, uint32_t world) {
    size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; l < n; l += stride) {
        const size_t i = Stripes{rank, world}.global_index(l);
        fe_t acc;
        if (AFFINE) {
            const fe_t w0 = a.w[0][i];
            acc = w0;
            for (uint32_t j = 1; j < a.J; ++j) acc = F::add(acc, F::mul(a.coef[j], F::sub(a.w[j][i], w0)));
        } else {
            acc = F::mul(a.coef[0], a.w[0][i]);
            for (uint32_t j = 1; j < a.J; ++j) acc = F::add(acc, F::mul(a.coef[j], a.w[j][i]));
        }
        out[i] = acc;
    }
}

// the same sum on listed rows of every column (the halo rows of a sharded fold): element c * col_len + rows[i]
template <class F>
__global__ void k_lincomb_rows(fe_t *__restrict__ out, LincombArgs a, const uint32_t *__restrict__ rows, size_t n_rows, size_t cols, size_t col_len) {
    size_t l = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= n_rows * cols) return;
    const size_t i = (l / n_rows) * col_len + rows[l % n_rows];
    fe_t acc = F::mul(a.coef[0], a.w[0][i]);
    for (uint32_t j = 1; j < a.J; ++j) acc = F::add(acc, F::mul(a.coef[j], a.w[j][i]));
    out[i] = acc;
}

// ---- folds ----
template <class F>
__global__ void k_fold_w(fe_t *__restrict__ out, const fe_t *__restrict__ w1, const fe_t *__restrict__ w2, fe_t r, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) out[i] = F::add(w1[i], F::mul(r, w2[i]));
}
struct FoldEArgs {
    const fe_t *t[DMAX];
    fe_t rpow[DMAX];
    uint32_t n_terms;
};
template <class F>
__global__ void k_fold_e(fe_t *out, const fe_t *e, FoldEArgs fa, size_t n) {   // out may alias e
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        fe_t acc = e[i];
#pragma unroll
        for (uint32_t k = 0; k < DMAX; ++k)
            if (k < fa.n_terms) acc = F::add(acc, F::mul(fa.rpow[k], fa.t[k][i]));
        out[i] = acc;
    }
}

// the translation unit hiprtc compiles: the emitted program `jit_fn` wrapped in the kernel body the ahead-of-time kernels use
static std::string jit_translation_unit(const std::string &fn_source, int field, bool has_sweep = false) {
    const std::string fname = field == 0 ? "Fr" : "Fq";
    std::string body;
    if (has_sweep)      // same choice as k_rowprog_spec: sweep form whenever the advice leaves are affine in the point
        body = "    if (A.ctx.wcoef == nullptr && A.npts <= DMAX + 1) {\n        sweep_kernel_body<" + fname +
               ">(A, jit_fn_sweep_one<" + fname + ">(), [](const RowCtx &C, uint32_t row, uint32_t npts, const fe_t *U, uint32_t nu, uint32_t *acc, "
               "bool accumulate) { jit_fn_sweep<" + fname + ">(C, row, npts, U, nu, acc, accumulate); });\n        return;\n    }\n";
    return "#include \"rowprog_dev.cuh\"\nnamespace srs {\nnamespace rowprog {\n" + fn_source +
           "extern \"C\" __global__ void __launch_bounds__(128, 2) srs_jit_rowprog(DevArgs A) {\n" + body + "    spec_kernel_body<" + fname +
           ">(A, [](const RowCtx &C, uint32_t row, uint32_t pt, const fe_t *U) { return jit_fn<" + fname + ">(C, row, pt, U); });\n}\n}\n}\n";
}

// The translation unit of a gate set's ProtoGalaxy leaf kernels: `fn_sources` holds, per gate g, the emitted program pg_jit_fn_<g>
// (emit_spec_source) and, with `sweep`, its sweep form pg_jit_fn_<g>_sweep (emit_sweep_source).  A dispatcher over the gate -- the
// PgSpecCall of tools/gen_rowprog_spec.py, a switch on the wave-uniform gate index -- and extern "C" kernels over the bodies the
// ahead-of-time kernels use (rowprog_dev.cuh): the leaves in `run` form, the leaves in sweep form (intended rows only: the reference's
// rows of such a structure stay on the hoisted interpreter pass), and F's leaf cubics (sweep form with one point when there is one).
static std::string pg_leaf_unit(const std::string &fn_sources, size_t n_gates, bool sweep, int waves) {
    const std::string bounds = "__launch_bounds__(128, " + std::to_string(waves == 1 ? 1 : 2) + ")";
    auto chain = [&](const std::string &ret, const std::string &suffix, const std::string &args) {
        std::string o = "        switch (gate) {\n";
        for (size_t g = 0; g + 1 < n_gates; ++g)
            o += "        case " + std::to_string(g) + ": " + ret + "pg_jit_fn_" + std::to_string(g) + suffix + "<Fr>(" + args + ");" + (ret.empty() ? " return;" : "") + "\n";
        return o + "        default: " + ret + "pg_jit_fn_" + std::to_string(n_gates - 1) + suffix + "<Fr>(" + args + ");\n        }\n";
    };
    std::string o = "#include \"rowprog_dev.cuh\"\nnamespace srs {\nnamespace rowprog {\n" + fn_sources + "struct PgJitCall {\n"
                    "    static __device__ __forceinline__ fe_t run(uint32_t gate, const RowCtx &C, uint32_t row, uint32_t pt, const fe_t *U) {\n" +
                    chain("return ", "", "C, row, pt, U") + "    }\n";
    if (sweep)
        o += "    static __device__ __forceinline__ void sweep(uint32_t gate, const RowCtx &C, uint32_t row, uint32_t npts, const fe_t *U, uint32_t nu, "
             "uint32_t *acc, bool accumulate) {\n" + chain("", "_sweep", "C, row, npts, U, nu, acc, accumulate") + "    }\n"
             "    static __device__ __forceinline__ uint32_t one(uint32_t gate) {\n" + chain("return ", "_sweep_one", "") + "    }\n";
    o += "};\n"
         "extern \"C\" __global__ void " + bounds + " srs_pg_jit_leaves_run(PgArgs A) {\n"
         "    __shared__ fe_t red[RP_THREADS];\n    pg_leaves_spec_body<Fr, PgJitCall, 8>(A, red);\n}\n";
    if (sweep)
        o += "extern \"C\" __global__ void " + bounds + " srs_pg_jit_leaves_sweep(PgArgs A) {\n"
             "    __shared__ fe_t red[RP_THREADS];\n    SRS_SWEEP_ACC(acc_all);\n    pg_leaves_sweep_body<Fr, PgJitCall, 8, false>(A, red, acc_all);\n}\n";
    o += "extern \"C\" __global__ void __launch_bounds__(128, 1) srs_pg_jit_F_leaves(PgFArgs B) {\n";
    if (sweep)
        o += "    __shared__ uint32_t acc[SW_WORDS * RP_THREADS];\n"
             "    pg_F_leaves_body<Fr>(B.A, B.Lv, B.nodes, B.n_nodes, PgFLeafSweep<Fr, PgJitCall>{acc + threadIdx.x});\n";
    else
        o += "    pg_F_leaves_body<Fr>(B.A, B.Lv, B.nodes, B.n_nodes, PgFLeafRun<Fr, PgJitCall>{});\n";
    return o + "}\n}\n}\n";
}

// ... of a structure's gate programs.  Only when EVERY gate has a sweep form does the unit carry the sweep-form kernels.
std::string pg_leaf_unit_source(const Compiled &c, bool *sweep_form, int waves) {
    bool sweep = !c.gate_progs.empty();
    for (const Program &gp : c.gate_progs) sweep = sweep && gp.sweep_ok;
    std::string fns;
    for (size_t g = 0; g < c.gate_progs.size(); ++g) {
        const std::string name = "pg_jit_fn_" + std::to_string(g);
        fns += emit_spec_source(c.gate_progs[g], name, true);
        if (sweep) fns += emit_sweep_source(c.gate_progs[g], name + "_sweep", true);
    }
    if (sweep_form) *sweep_form = sweep;
    return pg_leaf_unit(fns, c.gate_progs.size(), sweep, waves);
}
std::string cross_unit_source(const Compiled &c, int field) {
    return jit_translation_unit(emit_spec_source(c.cross, "jit_fn", true) + emit_sweep_source(c.cross, "jit_fn_sweep", true), field, c.cross.sweep_ok);
}
size_t pg_leaf_unit_insns(const Compiled &c) {
    size_t n = 0;
    for (const Program &gp : c.gate_progs) n += gp.vins.size();
    return n;
}

// Host-only check of the run-time compilation path (no device): a small program in the emitted form -- column loads,
// called and inlined multipliers, a uniform -- must compile with hiprtc against the headers embedded in the library.
bool jit_selfcheck(size_t *code_bytes, std::string &log) {
    const std::string fn =
        "template <class F>\n__device__ __forceinline__ fe_t jit_fn(const RowCtx &C, uint32_t row, uint32_t pt, const fe_t *__restrict__ U) {\n"
        "    const uint32_t mask = C.rows - 1;\n"
        "    const fe_t v0 = ld_fix<F>(C, 0, (row + 0u) & mask);\n"
        "    const fe_t v1 = ld_adv<F>(C, 0, (row + 1u) & mask, pt);\n"
        "    const fe_t v2 = ld_sel<F>(C, 0, (row + 0u) & mask);\n"
        "    const fe_t v3 = mul_ni<F>(v0, v1);\n"
        "    const fe_t v4 = sqr_ni<F>(v3);\n"
        "    const fe_t v5 = F::mul(U[0], v2);\n"
        "    return F::sub(F::add(v4, v5), F::dbl(F::neg(v1)));\n}\n"
        // and one in sweep form: affine advice leaf, called 9 x 29-bit multipliers, lazy add / sub, closing product
        "template <class F> __device__ constexpr uint32_t jit_fn_sweep_one() { return 1u; }\n"
        "template <class F>\n__device__ __forceinline__ void jit_fn_sweep(const RowCtx &C, uint32_t row, uint32_t npts, const fe_t *__restrict__ Uall, "
        "uint32_t nu, uint32_t *__restrict__ acc, bool accumulate) {\n"
        "    using G = Fp29<typename F::Params>;\n    const uint32_t mask = C.rows - 1;\n"
        "    const fe_t l0 = ld_fix<F>(C, 0, (row + 0u) & mask);\n"
        "    fe_t l1, s1; adv_affine<F>(C, 0, (row + 1u) & mask, l1, s1);\n"
        "    for (uint32_t pt = 0; pt < npts; ++pt) {\n"
        "        const fe_t *__restrict__ U = Uall + (size_t)pt * nu;\n"
        "        const f29_t x0 = G::unpack(l0), x1 = G::unpack(l1);\n"
        "        const f29_t x2 = mul29_ni<F>(x0, x1);\n"
        "        const f29_t x3 = sqr29_ni<F>(x2);\n"
        "        const f29_t x4 = G::normalize(G::template sub_lazy<3, 0>(G::normalize(G::add_lazy(x3, x2)), x3));\n"
        "        const f29_t x5 = G::mul(x4, G::unpack(U[0]));\n"
        "        sw_store(acc, pt, accumulate ? G::normalize(G::add_lazy(sw_load(acc, pt), x5)) : x5);\n"
        "        l1 = F::add(l1, s1);\n    }\n}\n";
    for (int field = 0; field < 2; ++field) {
        size_t bytes = 0;
        if (!jit::compile_only(jit_translation_unit(fn, field, true), &bytes, log)) return false;
        if (code_bytes) *code_bytes = bytes;
    }
    // ... and the ProtoGalaxy leaf unit (pg_leaf_unit: dispatcher and the three kernels over the bodies of rowprog_dev.cuh) of a canned
    // two-gate set made of the same program, with the sweep form and without
    auto renamed = [&](const std::string &to) {
        std::string t = fn;
        for (size_t at = 0; (at = t.find("jit_fn", at)) != std::string::npos; at += to.size()) t.replace(at, 6, to);
        return t;
    };
    const std::string two = renamed("pg_jit_fn_0") + renamed("pg_jit_fn_1");
    for (int sweep = 1; sweep >= 0; --sweep)
        if (!jit::compile_only(pg_leaf_unit(two, 2, sweep != 0, 1 + sweep), nullptr, log)) return false;
    return true;
}

struct Structure : Compiled {     // Compiled (rowprog_compile.h): the programs, degrees and Vandermonde matrices derived from the expressions
    int field = 0;
    uint32_t k = 0;
    size_t rows = 0, num_selectors = 0, num_fixed = 0, num_advice = 0;
    size_t num_lookups = 0;        // lookup arguments (src/plonk/lookup.rs:72-82); 5 fold variables each
    bool has_vector_lookup = false;
    int pg_spec_id = -1;           // ahead-of-time specialised leaf kernel for this gate set, or -1
    GateProg *d_gate_progs = nullptr;
    // the leaf kernels of this gate set compiled at run time (pg_jit_ensure): one module, pg_jit_run owns it; pg_jit_sweep only when every
    // gate has a sweep form.  pg_jit_state: 0 not tried, 1 loaded, -1 the compile or the load failed (pg_jit_log; the interpreter stays)
    jit::Kernel pg_jit_run, pg_jit_sweep, pg_jit_F;
    int pg_jit_state = 0;
    std::string pg_jit_log;
    // device data
    uint8_t **d_sel_ptrs = nullptr;
    fe_t **d_fix_ptrs = nullptr;
    std::vector<void *> owned;
    fe_t *d_vinv = nullptr, *d_vinv29 = nullptr;
    fe_t *d_kM[2] = {nullptr, nullptr};      // pg_K_from_G_device: the full inverse Vandermonde matrix of the nodes 0..d_G / 1..d_G+1 (made on first use)
    Arena arena;
    Arena lookup_scratch;              // sps_lookup_round_1: the multiplicity tables of every lookup (grow-only)
    std::vector<uint8_t> host_stage;   // source of the per-call staging copy (must outlive the asynchronous copy)
    uint32_t shard_rank = 0, shard_world = 1;   // cross terms: evaluate only this rank's row stripes (set_shard)
};

// the ahead-of-time kernel of a program (index into launch_spec), or -1; taken by the fingerprint of the plain program
static int match_spec(const Program &p) {
    if (!p.sweep_ok) return -1;     // the ahead-of-time kernels ARE the sweep form
    int id = -1;
    for (size_t i = 0; i < sizeof(kSpecs) / sizeof(kSpecs[0]); ++i)
        if (kSpecs[i].fingerprint == p.fingerprint && kSpecs[i].id >= 0) id = kSpecs[i].id;
    return id;
}

// A device buffer of bytes + spare owned by the structure, holding the `bytes` at `src`: allocate, record in `owned`, then copy --
// a copy that throws leaves the buffer to destroy().
static void *resident(Structure &S, const void *src, size_t bytes, hipMemcpyKind kind = hipMemcpyHostToDevice, size_t spare = 0) {
    void *d = nullptr;
    SRS_HIP_CHECK(hipMalloc(&d, bytes + spare));
    S.owned.push_back(d);
    if (bytes) SRS_HIP_CHECK(hipMemcpy(d, src, bytes, kind));
    return d;
}

Structure *create(int field, uint32_t k, size_t num_selectors, size_t num_fixed, size_t num_advice,
                  const uint8_t *const *selectors, const fe_t *const *fixed, int space_device,
                  const uint64_t *gates, size_t gates_words, size_t num_gates, size_t num_lookups, bool has_vector_lookup,
                  const uint64_t *lookup_exprs, size_t lookup_words, int &rc, std::string &err) {
    // destroy(), not delete: an exception half-way (e.g. hipMalloc of the fixed columns at a large k) must free the device
    // allocations and the run-time compiled module the structure already owns; the early returns on a compile error rely
    // on it too (destroy() of a structure that owns nothing yet is harmless)
    std::unique_ptr<Structure, void (*)(Structure *)> S(new Structure(), &destroy);
    // ---- 1. the expressions -> programs (rc 4 / 7 on failure)
    if (!compile_structure(field, num_selectors, num_fixed, num_advice, gates, gates_words, num_gates, num_lookups, has_vector_lookup,
                           lookup_exprs, lookup_words, *S, rc, err))
        return nullptr;
    S->field = field;
    S->k = k;
    S->rows = (size_t)1 << k;
    S->num_selectors = num_selectors;
    S->num_fixed = num_fixed;
    S->num_advice = num_advice;
    S->num_lookups = num_lookups;
    S->has_vector_lookup = has_vector_lookup;
    // ---- 2. ahead-of-time kernels for these programs (rowprog_spec.inc)
    S->cross.spec_id = match_spec(S->cross);
    S->plain_compressed.spec_id = match_spec(S->plain_compressed);
    S->plain_homogeneous.spec_id = match_spec(S->plain_homogeneous);
    for (auto &gp : S->gate_progs) gp.spec_id = match_spec(gp);
    for (auto &lp : S->lookup_progs) lp.spec_id = match_spec(lp);
    for (size_t e = 0; e < sizeof(kPgSpecs) / sizeof(kPgSpecs[0]); ++e) {
        if ((size_t)kPgSpecs[e].n_gates != S->gate_progs.size()) continue;
        bool same = true;
        for (size_t g = 0; g < S->gate_progs.size(); ++g) same = same && kPgSpecs[e].fp[g] == S->gate_progs[g].fingerprint;
        for (size_t g = 0; g < S->gate_progs.size(); ++g) same = same && S->gate_progs[g].sweep_ok;      // the leaf kernels use the sweep form
        if (same) S->pg_spec_id = kPgSpecs[e].id;
    }
    // ---- 3. no ahead-of-time kernel for this gate set: compile the cross-term program now (jit.hip).  Worth it from 2^14
    //      rows on (one hiprtc compile ~ a second); single-pass degrees only (the kernel body parks d + 1 <= 9 points).
    if (S->cross.spec_id < 0 && S->degree >= 1 && S->degree <= DMAX && !S->cross.insns.empty() && jit::enabled() &&
        (k >= 14 || tuning::get_or(tuning::JIT_ALWAYS, 0) != 0)) {
        const bool shared = true;
        const std::string src = jit_translation_unit(emit_spec_source(S->cross, "jit_fn", shared) + emit_sweep_source(S->cross, "jit_fn_sweep", shared),
                                                     field, S->cross.sweep_ok);
        std::string log;
        (void)jit::compile(src, "srs_jit_rowprog", S->cross.jit, log);      // on failure the structure stays on the interpreter (srs_structure_jit_info reports which)
    }
    // ---- 4. device residency: programs, fixed columns, selectors
    rc = 5;
    auto upload_program = [&](Program &p) {
        if (!p.insns.empty()) p.d_insns = (Insn *)resident(*S, p.insns.data(), p.insns.size() * sizeof(Insn));
    };
    for (auto &lp : S->lookup_progs) upload_program(lp);
    upload_program(S->cross);
    upload_program(S->plain_compressed);
    upload_program(S->plain_homogeneous);
    for (auto &gp : S->gate_progs) upload_program(gp);
    if (!S->vinv.empty()) {
        S->d_vinv = (fe_t *)resident(*S, S->vinv.data(), S->vinv.size() * sizeof(fe_t));
        const FieldOps f{field};
        std::vector<fe_t> v29(S->vinv);                        // * 2^5: operands of the 2^261-radix multiplier (sweep_kernel_body)
        for (auto &x : v29)
            for (int k = 0; k < 5; ++k) x = f.add(x, x);
        S->d_vinv29 = (fe_t *)resident(*S, v29.data(), v29.size() * sizeof(fe_t));
    }
    const hipMemcpyKind kind = space_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    std::vector<uint8_t *> selp(num_selectors);
    std::vector<fe_t *> fixp(num_fixed);
    for (size_t i = 0; i < num_selectors; ++i) selp[i] = (uint8_t *)resident(*S, selectors[i], S->rows, kind);
    for (size_t i = 0; i < num_fixed; ++i) fixp[i] = (fe_t *)resident(*S, fixed[i], S->rows * sizeof(fe_t), kind);
    // the pointer tables keep one spare entry: never an empty allocation
    S->d_sel_ptrs = (uint8_t **)resident(*S, selp.data(), num_selectors * sizeof(void *), hipMemcpyHostToDevice, sizeof(void *));
    S->d_fix_ptrs = (fe_t **)resident(*S, fixp.data(), num_fixed * sizeof(void *), hipMemcpyHostToDevice, sizeof(void *));
    rc = 0;
    return S.release();
}

void destroy(Structure *S) {
    if (!S) return;
    jit::release(S->cross.jit);
    jit::release(S->pg_jit_sweep);
    jit::release(S->pg_jit_F);
    jit::release(S->pg_jit_run);          // the module of all three
    for (void *p : S->owned) (void)hipFree(p);
    S->arena.release();
    S->lookup_scratch.release();
    delete S;
}

void set_shard(Structure *S, uint32_t rank, uint32_t world) {
    S->shard_rank = rank;
    S->shard_world = world ? world : 1;
}
uint32_t shard_world(const Structure *S) { return S->shard_world; }
uint32_t shard_rank(const Structure *S) { return S->shard_rank; }
void rotation_range(const Structure *S, int32_t *lo, int32_t *hi) { *lo = S->min_rot; *hi = S->max_rot; }
uint32_t log_rows(const Structure *S) { return S->k; }
size_t degree(const Structure *S) { return S->degree; }
size_t num_challenges(const Structure *S) { return S->s_num_challenges; }
size_t num_advice(const Structure *S) { return S->num_advice; }
size_t num_witness_columns(const Structure *S) { return S->num_advice + 5 * S->num_lookups; }
size_t num_lookups(const Structure *S) { return S->num_lookups; }
bool has_vector_lookup(const Structure *S) { return S->has_vector_lookup; }
size_t rows(const Structure *S) { return S->rows; }
size_t num_gates(const Structure *S) { return S->gate_progs.size(); }
int field(const Structure *S) { return S->field; }

template <class F>
static void launch_rowprog(const DevArgs &A, uint32_t nslots, hipStream_t st) {
    uint32_t blocks = (A.ctx.local_rows + RP_THREADS - 1) / RP_THREADS;
    if (nslots <= 8) SRS_LAUNCH((k_rowprog<F, 8>), (blocks), (RP_THREADS), 0, st, A);
    else if (nslots <= 10) SRS_LAUNCH((k_rowprog<F, 10>), (blocks), (RP_THREADS), 0, st, A);
    else if (nslots <= 12) SRS_LAUNCH((k_rowprog<F, 12>), (blocks), (RP_THREADS), 0, st, A);
    else if (nslots <= 16) SRS_LAUNCH((k_rowprog<F, 16>), (blocks), (RP_THREADS), 0, st, A);
    else if (nslots <= 24) SRS_LAUNCH((k_rowprog<F, 24>), (blocks), (RP_THREADS), 0, st, A);
    else SRS_LAUNCH((k_rowprog<F, 32>), (blocks), (RP_THREADS), 0, st, A);
}

// 0 interpreter, 1 ahead-of-time specialised kernel, 2 compiled at run time (include/sirius_amd.h SRS_KERNEL_*)
// ---- ProtoGalaxy leaf kernels compiled at run time
// The leaf kernels a call takes: 1 ahead of time, 2 compiled at run time, 0 interpreter.  The compiled ones serve the intended leaf rows
// only (compat == 0): the reference's rows make every leaf of a gate one value, which the hoisted interpreter pass evaluates once.
static int pg_leaf_kind(const Structure *S, int compat) {
    if (!compat && S->pg_jit_run.function && (S->pg_spec_id < 0 || tuning::get_or(tuning::PG_JIT_FORCE, 0) != 0)) return 2;
    return S->pg_spec_id >= 0 ? 1 : 0;
}
// ... and whether they include the sweep form (integer-point G, e, F's leaves)
static bool pg_leaf_sweep_form(const Structure *S, int compat) {
    const int kind = pg_leaf_kind(S, compat);
    return kind == 1 || (kind == 2 && S->pg_jit_sweep.function != nullptr);
}
// A leaf unit inlines every gate program 8 times per kernel (the 8 leaves of a thread); hiprtc's time grows linearly with the summed SSA
// instruction count of the gates, 1.4 - 2.1 times that of a cross-term unit of the same size (profiles/pg_leaves_jit_ab.txt).  The cap
// is the size of the largest cross-term unit the library compiles at creation (degree 8: 4 x MainGate<5>, 313 instructions): a leaf
// unit never takes more than about twice that one; above it the structure stays on the interpreter.
constexpr size_t PG_JIT_MAX_INSNS = 320;
// The two leaf kernels of a unit are bounded for two waves per SIMD (256 VGPRs), as the ahead-of-time ones; a unit of more than
// PG_JIT_ONE_WAVE_INSNS instructions for one (512): large gate programs spill at 256 (profiles/pg_leaves_jit_ab.txt).  Tuning
// pg_jit_waves overrides the choice.
constexpr size_t PG_JIT_ONE_WAVE_INSNS = PG_JIT_MAX_INSNS;      // no unit below the cap measured faster at one wave
static int pg_jit_waves(const Structure *S) {
    const int64_t t = tuning::get_or(tuning::PG_JIT_WAVES, 0);
    if (t == 1 || t == 2) return (int)t;
    return pg_leaf_unit_insns(*S) > PG_JIT_ONE_WAVE_INSNS ? 1 : 2;
}
// Whether the structure may get compiled leaf kernels; `lazy`: asked by a call that is about to run leaves over rows (then only
// from 2^14 rows on, the rule of the cross terms), else by srs_structure_prepare_pg_leaves.
static bool pg_jit_allowed(const Structure *S, bool lazy, std::string &why) {
    if (S->field != 0) { why = "ProtoGalaxy leaves exist for bn256::Fr only"; return false; }
    if (S->gate_progs.empty()) { why = "the structure has no gates"; return false; }
    if (S->k < 10) { why = "fewer than 2^10 rows: the leaf kernels map 8 leaves to a thread from 2^10 rows on"; return false; }
    if (!jit::enabled()) { why = "run-time compilation is disabled (tuning no_jit / SRS_NO_JIT)"; return false; }
    if (lazy && S->k < 14 && tuning::get_or(tuning::JIT_ALWAYS, 0) == 0) { why = "fewer than 2^14 rows"; return false; }
    const size_t insns = pg_leaf_unit_insns(*S);
    if (insns > PG_JIT_MAX_INSNS) {
        why = "the gate programs have " + std::to_string(insns) + " instructions, more than the " + std::to_string(PG_JIT_MAX_INSNS) +
              " a leaf unit is compiled for: the leaves stay on the interpreter";
        return false;
    }
    return true;
}
// Compiles and loads the leaf unit once per structure.  rc 0: compiled (now or earlier) or ahead-of-time kernels; 10: the rule excludes
// the structure (err says why); 4: the compile failed (err = the compiler's log; the structure stays on the interpreter).
int pg_jit_ensure(Structure *S, bool lazy, double *compile_seconds, std::string &err) {
    if (compile_seconds) *compile_seconds = 0;
    if (S->pg_spec_id >= 0 && tuning::get_or(tuning::PG_JIT_FORCE, 0) == 0) return 0;
    if (S->pg_jit_state > 0) return 0;
    if (S->pg_jit_state < 0) { err = S->pg_jit_log; return 4; }
    if (!pg_jit_allowed(S, lazy, err)) return 10;
    bool sweep = false;
    const std::string src = pg_leaf_unit_source(*S, &sweep, pg_jit_waves(S));
    std::string log;
    bool ok = jit::compile_unit(src, "srs_pg_jit_leaves_run", S->pg_jit_run, log) && jit::entry(S->pg_jit_run, "srs_pg_jit_F_leaves", S->pg_jit_F, log) &&
              (!sweep || jit::entry(S->pg_jit_run, "srs_pg_jit_leaves_sweep", S->pg_jit_sweep, log));
    if (compile_seconds) *compile_seconds = S->pg_jit_run.compile_seconds;
    if (!ok) {
        jit::release(S->pg_jit_sweep);
        jit::release(S->pg_jit_F);
        jit::release(S->pg_jit_run);
        S->pg_jit_state = -1;
        S->pg_jit_log = err = log.empty() ? "run-time compilation of the leaf kernels failed" : log;
        return 4;
    }
    S->pg_jit_state = 1;
    return 0;
}

int kernel_kind(const Structure *S, int which) {
    if (which == 2) return pg_leaf_kind(S, 0);
    const Program &p = which == 0 ? S->cross : S->plain_compressed;
    if (p.spec_id >= 0) return 1;
    if (p.jit.function) return 2;
    return 0;
}

const char *spec_source(Structure *S, int which, uint64_t *fingerprint, int *spec_id, std::string &buf) {
    if (which >= 3 && (size_t)(which - 3) >= S->gate_progs.size()) { buf.clear(); return buf.c_str(); }
    Program &p = which >= 3 ? S->gate_progs[which - 3] : (which == 0 ? S->cross : (which == 1 ? S->plain_compressed : S->plain_homogeneous));
    buf = emit_spec_source(p, "spec_fn", false);   // ahead-of-time generation: inlined multipliers
    buf += emit_sweep_source(p, "spec_fn_sweep", false);  // empty when the program has no sweep form
    if (fingerprint) *fingerprint = p.fingerprint;
    if (spec_id) *spec_id = p.spec_id;
    if (spec_id && p.spec_id < 0 && p.jit.function) *spec_id = -2;      // compiled at run time
    return buf.c_str();
}

// mode 0: cross terms (needs W2), outputs `degree` vectors; mode 1/2: plain evaluation of the
// compressed / homogeneous expression on W1, one output vector.
static int evaluate_prog(Structure *S, Program &p, int mode, const fe_t *W1_dev, const fe_t *W2_dev, const fe_t *challenges_host,
                         size_t n_ch, fe_t *const *out_dev_ptrs_host, hipStream_t st, std::string &err, bool sync = true);
// sync = false: the kernels are only enqueued; the caller synchronises `st` before the next call on this structure
// (the uniform tables live in the structure's arena).  Used when an MSM over the outputs follows on the same stream.
int evaluate(Structure *S, int mode, const fe_t *W1_dev, const fe_t *W2_dev, const fe_t *challenges_host, size_t n_ch,
             fe_t *const *out_dev_ptrs_host, hipStream_t st, std::string &err, bool sync) {
    Program &p = mode == 0 ? S->cross : (mode == 1 ? S->plain_compressed : S->plain_homogeneous);
    return evaluate_prog(S, p, mode, W1_dev, W2_dev, challenges_host, n_ch, out_dev_ptrs_host, st, err, sync);
}
static int evaluate_prog(Structure *S, Program &p, int mode, const fe_t *W1_dev, const fe_t *W2_dev, const fe_t *challenges_host,
                         size_t n_ch, fe_t *const *out_dev_ptrs_host, hipStream_t st, std::string &err, bool sync) {
    FieldOps f{S->field};
    const uint32_t d = mode == 0 ? (uint32_t)S->degree : 0;
    const uint32_t npts = mode == 0 ? d + 1 : 1;
    const uint32_t nout = mode == 0 ? d : 1;
    if (mode == 0 && d == 0) return 0;
    if (p.nslots > 32) { err = "row program needs more than 32 live registers"; return 4; }
    const size_t nu = p.uops.size() ? p.uops.size() : 1;
    std::vector<fe_t> utab(nu * npts);
    for (uint32_t pt = 0; pt < npts; ++pt)
        if (!eval_uniform(p, f, challenges_host, n_ch, S->h_num_challenges, mode == 0, pt, utab.data() + (size_t)pt * nu, err)) return 7;
    // uniform tables and output pointers travel in ONE host-to-device copy (each small pageable copy costs ~50 us of
    // host time, during which the GPU idles)
    Arena &A = S->arena;
    const size_t utab_bytes = utab.size() * sizeof(fe_t), stage_bytes = utab_bytes + nout * sizeof(void *);
    A.reserve(Arena::pad(stage_bytes) + 1024);
    A.reset();
    uint8_t *d_stage = A.take<uint8_t>(stage_bytes);
    fe_t *d_utab = reinterpret_cast<fe_t *>(d_stage);
    fe_t **d_out = reinterpret_cast<fe_t **>(d_stage + utab_bytes);
    S->host_stage.resize(stage_bytes);
    std::memcpy(S->host_stage.data(), utab.data(), utab_bytes);
    std::memcpy(S->host_stage.data() + utab_bytes, out_dev_ptrs_host, nout * sizeof(void *));
    SRS_HIP_CHECK(hipMemcpyAsync(d_stage, S->host_stage.data(), stage_bytes, hipMemcpyHostToDevice, st));
    DevArgs a;
    a.prog = p.d_insns;
    a.n_insn = (uint32_t)p.insns.size();
    a.result = p.result;
    a.ctx.rows = (uint32_t)S->rows;
    a.ctx.sel = S->d_sel_ptrs;
    a.ctx.fix = S->d_fix_ptrs;
    for (uint32_t j = 0; j < JMAX; ++j) a.ctx.W[j] = nullptr;
    a.ctx.W[0] = W1_dev;
    a.ctx.W[1] = W2_dev;
    a.ctx.J = mode == 0 ? 2 : 1;
    a.ctx.wcoef = nullptr;
    a.ctx.half = 0;
    a.ctx.pt0 = 0;
    // only the cross terms are sharded (their consumers, the sharded MSM and the error fold, touch this rank's stripes
    // only); the deciders' plain evaluations always cover every row
    a.ctx.shard_rank = mode == 0 ? S->shard_rank : 0;
    a.ctx.shard_world = mode == 0 ? S->shard_world : 1;
    a.ctx.local_rows = (uint32_t)Stripes{a.ctx.shard_rank, a.ctx.shard_world}.count(S->rows);
    a.utab = d_utab;
    a.n_uniform = (uint32_t)nu;
    a.npts = npts;
    // d <= 8: one pass.  Higher folding degrees (many gates compressed with y^(n-1)): every pass evaluates all
    // d + 1 points again and accumulates the next 8 coefficients (a.d = outputs of THIS pass).
    for (uint32_t k0 = 0; k0 < (d ? d : 1); k0 += DMAX) {
        a.d = d ? std::min<uint32_t>(DMAX, d - k0) : 0;
        a.vinv = S->d_vinv ? S->d_vinv + (size_t)k0 * npts : nullptr;
        a.vinv29 = S->d_vinv29 ? S->d_vinv29 + (size_t)k0 * npts : nullptr;
        a.out = d_out + k0;
        prof::Scope ps(mode == 0 ? "rowprog_cross_terms" : "rowprog_eval", st, S->rows);
        if (p.spec_id >= 0) launch_spec(p.spec_id, S->field, a, st);
        else if (p.jit.function) {
            if (!jit::launch(p.jit, (a.ctx.local_rows + RP_THREADS - 1) / RP_THREADS, RP_THREADS, p.sweep_ok ? sweep_smem_bytes(a.npts) : 0u, &a, st)) {
                err = "launch of the run-time compiled row program failed";
                return 5;
            }
        }
        else if (S->field == 0) launch_rowprog<Fr>(a, p.nslots, st); else launch_rowprog<Fq>(a, p.nslots, st);
    }
    if (!sync) return 0;
    SRS_HIP_CHECK(hipStreamSynchronize(st));   // utab / pointer staging lives in the arena
    SRS_HIP_CHECK(hipGetLastError());
    prof::collect();
    return 0;
}

void fold_w(int field, fe_t *out, const fe_t *w1, const fe_t *w2, const fe_t &r, size_t n, hipStream_t st) {
    if (!n) return;
    uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, 256 * 16);
    if (field == 0) SRS_LAUNCH((k_fold_w<Fr>), (blocks), (256), 0, st, out, w1, w2, r, n);
    else SRS_LAUNCH((k_fold_w<Fq>), (blocks), (256), 0, st, out, w1, w2, r, n);
}

int fold_e(int field, fe_t *out, const fe_t *e, const fe_t *const *t_dev_ptrs_host, size_t n_terms, const fe_t &r, size_t n,
           hipStream_t st, std::string &err) {
    (void)err;
    FieldOps f{field};
    if (!n) return 0;
    uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, 256 * 16);
    fe_t acc = r;   // r^1, r^2, ...  (accumulator.rs:380-383)
    const fe_t *src = e;
    for (size_t k0 = 0; k0 == 0 || k0 < n_terms; k0 += DMAX) {      // 8 terms per launch; later launches accumulate onto out
        FoldEArgs fa;
        fa.n_terms = (uint32_t)std::min<size_t>(DMAX, n_terms - k0);
        for (uint32_t k = 0; k < DMAX; ++k) {
            fa.t[k] = k < fa.n_terms ? t_dev_ptrs_host[k0 + k] : nullptr;
            fa.rpow[k] = acc;
            if (k < fa.n_terms) acc = f.mul(acc, r);
        }
        if (field == 0) SRS_LAUNCH((k_fold_e<Fr>), (blocks), (256), 0, st, out, src, fa, n);
        else SRS_LAUNCH((k_fold_e<Fq>), (blocks), (256), 0, st, out, src, fa, n);
        src = out;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------
// ProtoGalaxy host side
// ---------------------------------------------------------------------------------------------
static size_t next_pow2(size_t v) { size_t p = 1; while (p < v) p <<= 1; return p; }
static uint32_t ilog2(size_t v) { uint32_t l = 0; while (((size_t)1 << (l + 1)) <= v) ++l; return l; }

// PolyContext (src/nifs/protogalaxy/poly/mod.rs:205-269)
bool pg_sizes(const Structure *S, size_t traces_len, PgSizes &o) {
    size_t count = S->rows * S->gate_progs.size();           // get_count_of_valuation :511-516
    if (count == 0) return false;
    o.count_with_padding = next_pow2(count);                   // :518-533
    o.betas_count = ilog2(o.count_with_padding);               // :237-239
    o.points_F = next_pow2(o.betas_count + 1);                 // :241-243
    o.instances_to_fold = traces_len + 1;
    o.points_G = next_pow2(traces_len * S->max_gate_degree + 1);   // get_points_count :535-545
    o.lagrange_domain = ilog2(o.instances_to_fold);            // :253-255
    // Q2: fft_log_domain_size_K returns a COUNT that is then used as a LOG (:263-268, :481)
    size_t c = o.points_G + 1;
    c = c > o.instances_to_fold ? c - o.instances_to_fold : 0;
    o.log_domain_K = (uint32_t)next_pow2(c);
    return true;
}

// iter_eval_lagrange_poly_for_cyclic_group (src/polynomial/lagrange.rs:50-75), Fr, host
std::vector<fe_t> lagrange_eval(const fe_t &X, uint32_t log_n) {
    const size_t n = (size_t)1 << log_n;
    fe_t w = ntt::omega(log_n, false);
    fe_t xn1 = Fr::sub(Fr::pow_u64(X, n), Fr::one());
    std::vector<fe_t> out(n), val(n), den(n), pre(n + 1);
    // one inversion for n and all the X - w^i (Montgomery's trick; a zero difference -- X on the domain -- is left out of the product)
    fe_t value = Fr::one(), acc = Fr::from_u64(n);
    pre[0] = acc;
    for (size_t i = 0; i < n; ++i) {
        val[i] = value;
        den[i] = Fr::sub(X, value);
        if (!Fr::is_zero(den[i])) acc = Fr::mul(acc, den[i]);
        pre[i + 1] = acc;
        value = Fr::mul(value, w);
    }
    fe_t inv = Fr::inv(acc);
    std::vector<fe_t> dinv(n);
    for (size_t i = n; i-- > 0;) {
        if (Fr::is_zero(den[i])) continue;
        dinv[i] = Fr::mul(inv, pre[i]);
        inv = Fr::mul(inv, den[i]);
    }
    const fe_t inv_n = inv;                                   // what is left: 1 / n
    for (size_t i = 0; i < n; ++i) {
        if (Fr::is_zero(den[i])) out[i] = Fr::is_zero(xn1) ? Fr::one() : Fr::zero();     // xn1 == 0 exactly when X is on the domain
        else out[i] = Fr::mul(Fr::mul(val[i], inv_n), Fr::mul(xn1, dinv[i]));
    }
    return out;
}

fe_t poly_eval(const fe_t *c, size_t n, const fe_t &x) {       // UnivariatePoly::eval (univariate.rs:67-75)
    fe_t acc = Fr::zero(), xp = Fr::one();
    for (size_t i = 0; i < n; ++i) {
        acc = Fr::add(acc, Fr::mul(xp, c[i]));
        xp = Fr::mul(xp, x);
    }
    return acc;
}

template <uint32_t NS>
static void launch_pg_leaves(const PgArgs &A, uint32_t tiles, uint32_t gates, uint32_t threads, uint32_t lpt, hipStream_t st) {
    if (lpt == 8) SRS_LAUNCH((k_pg_leaves<Fr, NS, 8>), (tiles, gates), (threads), 0, st, A);
    else SRS_LAUNCH((k_pg_leaves<Fr, NS, 1>), (tiles, gates), (threads), 0, st, A);
}

// ---------------------------------------------------------------------------------------------
// What the routes of the sums share: the evaluation points, the gates' uniform tables, the kernels' argument block,
// the leaf launches, the integer-node interpolation and the end of a call.  The routes themselves: pg_row0_values (closed form),
// pg_F_tree, pg_leaf_sums; pg_sum dispatches.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t PG_LPT = 8;      // leaves per thread once a gate has >= 1024 rows; the sweep kernels read their own table at slot PG_LPT

// what ends a call: the staging lives in the structure's arena until the stream has drained
static void finish(hipStream_t st) {
    SRS_HIP_CHECK(hipStreamSynchronize(st));
    SRS_HIP_CHECK(hipGetLastError());
    prof::collect();
}

static std::vector<fe_t> pg_deltas(const fe_t &delta, uint32_t levels) {      // delta^(2^b)  (:97-99)
    std::vector<fe_t> out(levels);
    fe_t d = delta;
    for (uint32_t b = 0; b < levels; ++b) { out[b] = d; d = Fr::sqr(d); }
    return out;
}

struct PgPoints {
    std::vector<fe_t> pts;                       // X_p: the integers pt0 .. pt0 + P - 1, or the P roots of unity (iter_cyclic_subgroup)
    std::vector<fe_t> wcoef;                     // fold: [P][J] = L_j(X_p)   (FoldedWitness::new, folded_witness.rs:20-47)
    std::vector<std::vector<fe_t>> ch_pt;        // the challenges per leaf point: fold ? the J traces' folded with L_j(X_p) : trace 0's
};
// fold = false (compute_F, evaluate_e): one leaf point on W_dev[0]; the P points are F's.  fold = true (compute_G): P leaf points
static PgPoints pg_points(bool g_int, uint32_t pt0, uint32_t P, bool fold, size_t J, uint32_t lagrange_domain, const fe_t *const *challenges_host,
                          size_t n_ch) {
    PgPoints o;
    const fe_t w = g_int || P == 1 ? Fr::one() : ntt::omega(ilog2(P), false);
    fe_t x = Fr::one();
    for (uint32_t p = 0; p < P; ++p) { o.pts.push_back(g_int ? Fr::from_u64(pt0 + p) : x); x = Fr::mul(x, w); }
    o.ch_pt.assign(fold ? P : 1, std::vector<fe_t>(n_ch ? n_ch : 1, Fr::zero()));
    if (!fold) {
        for (size_t c = 0; c < n_ch; ++c) o.ch_pt[0][c] = challenges_host[0][c];
        return o;
    }
    o.wcoef.resize((size_t)P * J);
    // integer-point G folds the witnesses by halvings in the kernel: L_j(X_p) is only needed to fold challenges
    for (uint32_t p = 0; p < P && (!g_int || n_ch); ++p) {
        std::vector<fe_t> L = lagrange_eval(o.pts[p], lagrange_domain);
        for (size_t j = 0; j < J; ++j) {
            o.wcoef[(size_t)p * J + j] = L[j];
            for (size_t c = 0; c < n_ch; ++c)                 // fold_plonk_challenges :142-180
                o.ch_pt[p][c] = Fr::add(o.ch_pt[p][c], Fr::mul(challenges_host[j][c], L[j]));
        }
    }
    return o;
}

// The sweep form of a gate's table (k_pg_leaves_sweep): PG_LPT + 1 tables.  Table 0 is the plain one; table l in [first, PG_LPT] holds the
// term coefficients (sw_coef) times w[l], one table per leaf slot of a thread -- or, not `weighted`, as they are: what row 0 (hoist_mode 1)
// reads at table PG_LPT.  The tables below `first` stay zero.
struct PgSlotWeights { uint32_t first; bool weighted; fe_t w[PG_LPT + 1]; };
// the leaf pass: w_l = prod_{b in bits(l)} c[b], c = the weights of the three levels a thread reduces in registers; table PG_LPT: the SUM of
// the w_l, l = 0 .. PG_LPT - 1 (reference_compat: the leaves of a thread share one evaluation at row 0)
static PgSlotWeights pg_slot_weights_leaves(const fe_t *c) {
    PgSlotWeights s;
    s.first = 1;
    s.weighted = true;
    fe_t wsum = Fr::one();
    for (uint32_t l = 1; l < PG_LPT; ++l) {
        fe_t wl = Fr::one();
        for (uint32_t b = 0; b < 3; ++b)
            if ((l >> b) & 1u) wl = Fr::mul(wl, c[b]);
        s.w[l] = wl;
        wsum = Fr::add(wsum, wl);
    }
    s.w[0] = Fr::one();
    s.w[PG_LPT] = wsum;
    return s;
}

struct PgGateTable {
    std::vector<GateProg> gp;
    std::vector<fe_t> utab;                      // per gate: [sw ? PG_LPT + 1 : 1][leaf points][n_uniform]
    uint32_t max_slots = 1;
};
// gp[], utab and max_slots of the structure's gates for the challenges ch_pt[leaf point]; sw: the sweep form, or nullptr
static int pg_gate_table(Structure *S, const std::vector<std::vector<fe_t>> &ch_pt, size_t n_ch, const PgSlotWeights *sw, PgGateTable &t, std::string &err) {
    FieldOps f{0};
    const uint32_t n_gates = (uint32_t)S->gate_progs.size(), leaf_pts = (uint32_t)ch_pt.size();
    t.gp.resize(n_gates);
    for (uint32_t g = 0; g < n_gates; ++g) {
        Program &p = S->gate_progs[g];
        GateProg &gp = t.gp[g];
        t.max_slots = std::max(t.max_slots, p.nslots);
        const size_t nu = p.uops.size() ? p.uops.size() : 1;
        gp.prog = p.d_insns;
        gp.n_insn = (uint32_t)p.insns.size();
        gp.result = p.result;
        gp.n_uniform = (uint32_t)nu;
        gp.utab_off = (uint32_t)t.utab.size();
        t.utab.resize(t.utab.size() + nu * leaf_pts * (sw ? PG_LPT + 1 : 1u));
        fe_t *tab = t.utab.data() + gp.utab_off;
        for (uint32_t lp = 0; lp < leaf_pts; ++lp)
            if (!eval_uniform(p, f, ch_pt[lp].data(), n_ch, 0, false, 0, tab + (size_t)lp * nu, err)) return 7;
        for (uint32_t l = sw ? sw->first : PG_LPT + 1; l <= PG_LPT; ++l) {
            fe_t *dst = tab + (size_t)l * leaf_pts * nu;
            std::memcpy(dst, tab, (size_t)leaf_pts * nu * sizeof(fe_t));
            for (uint32_t lp = 0; lp < leaf_pts && sw->weighted; ++lp)
                for (int ci : p.sw_coef) dst[(size_t)lp * nu + ci] = Fr::mul(dst[(size_t)lp * nu + ci], sw->w[l]);
        }
    }
    if (t.max_slots > 32) { err = "row program needs more than 32 live registers"; return 4; }
    return 0;
}

struct PgCall {                                  // what the callers of pg_args differ in
    size_t n_w = 1;                              // witness pointers handed over
    uint32_t J = 1;                              // witnesses folded at every leaf point (compute_G), else 1
    const fe_t *wcoef = nullptr;                 // device [P][J] = L_j(X_p); nullptr: no fold, or the fold by halvings (`half`)
    uint32_t half = 0, pt0 = 0;                  // integer-point G: the nodes pt0, pt0 + 1, ..
    int compat = 1;
    uint32_t leaf_pts = 1, P = 1, wpts = 1, tile_log = 0;
    const fe_t *weights = nullptr;
    fe_t *partial = nullptr, *hoist = nullptr;
    bool sharded = false;
};
// The kernels' argument block.  A row-sharded structure (set_shard), one rule, three callers:
//   pg_row0_values: unsharded -- every rank holds row 0, and pg_sum answers for the ranks >= 1 without a launch.
//   pg_F_tree, and pg_leaf_sums at k >= 10 (tile_log == STRIPE_LOG, a tile IS a stripe): the structure's rank and world -- this rank's tiles.
//   pg_leaf_sums with smaller tiles: rank 0 evaluates everything, no tile belongs to the other ranks.
// The rows themselves (ctx) are never sharded here: a tile reads all of its rows.
static PgArgs pg_args(const Structure *S, const fe_t *const *W_dev, const GateProg *d_gp, const fe_t *d_utab, const PgCall &c) {
    PgArgs a;
    a.gates = d_gp;
    a.n_gates = (uint32_t)S->gate_progs.size();
    a.log_rows = S->k;
    a.ctx.rows = (uint32_t)S->rows;
    a.ctx.sel = S->d_sel_ptrs;
    a.ctx.fix = S->d_fix_ptrs;
    for (uint32_t j = 0; j < JMAX; ++j) a.ctx.W[j] = j < c.n_w ? W_dev[j] : nullptr;
    a.ctx.J = c.J;
    a.ctx.wcoef = c.wcoef;
    a.ctx.half = c.half;
    a.ctx.pt0 = c.pt0;
    a.ctx.shard_rank = 0;
    a.ctx.shard_world = 1;
    a.ctx.local_rows = a.ctx.rows;
    a.compat = c.compat;
    a.leaf_pts = c.leaf_pts;
    a.P = c.P;
    a.utab = d_utab;
    a.weights = c.weights;
    a.wpts = c.wpts;
    a.tile_log = c.tile_log;
    a.partial = c.partial;
    a.shard_rank = 0;
    a.shard_world = 1;
    if (c.sharded && c.tile_log == STRIPE_LOG) { a.shard_rank = S->shard_rank; a.shard_world = S->shard_world; }
    else if (c.sharded && S->shard_world > 1 && S->shard_rank != 0) { a.shard_rank = 0xFFFFFFFFu; a.shard_world = 2; }     // no tile is mine
    a.hoist = c.hoist;
    a.hoist_mode = 0;
    return a;
}

// one leaf launch: the ahead-of-time gate set (8 leaves per thread only; sweep: its sweep form), else the interpreter by live registers
static void launch_leaves(const Structure *S, const PgArgs &a, uint32_t tiles, uint32_t threads, uint32_t lpt, uint32_t max_slots, bool sweep,
                          hipStream_t st) {
    const int kind = lpt == PG_LPT ? pg_leaf_kind(S, a.compat) : 0;
    if (kind == 2) {
        if (!jit::launch_grid(sweep ? S->pg_jit_sweep : S->pg_jit_run, tiles, a.n_gates, threads, sweep ? sweep_smem_bytes(a.P) : 0u, &a, st))
        { set_error("launch of the run-time compiled ProtoGalaxy leaf kernel failed"); throw DeviceError{5}; }
    }
    else if (kind == 1) launch_pg_spec(S->pg_spec_id, a, tiles, a.n_gates, threads, st, sweep);
    else if (max_slots <= 8) launch_pg_leaves<8>(a, tiles, a.n_gates, threads, lpt, st);
    else if (max_slots <= 12) launch_pg_leaves<12>(a, tiles, a.n_gates, threads, lpt, st);
    else if (max_slots <= 16) launch_pg_leaves<16>(a, tiles, a.n_gates, threads, lpt, st);
    else launch_pg_leaves<32>(a, tiles, a.n_gates, threads, lpt, st);
}

static void launch_F_leaves(const Structure *S, const PgArgs &a, const PgFLevels &lv, uint32_t tiles, uint32_t threads, uint32_t max_slots, fe_t *out,
                            uint32_t n0, hipStream_t st) {
    if (pg_leaf_kind(S, a.compat) == 2) {
        const PgFArgs fa{a, lv, out, n0};
        if (!jit::launch_grid(S->pg_jit_F, tiles, a.n_gates, threads, 0u, &fa, st)) { set_error("launch of the run-time compiled ProtoGalaxy F leaf kernel failed"); throw DeviceError{5}; }
    }
    else if (S->pg_spec_id == 0) SRS_LAUNCH((k_pg_F_leaves<Fr, 2, 0>), (tiles, a.n_gates), (threads), 0, st, a, lv, out, n0);
    else if (max_slots <= 8) SRS_LAUNCH((k_pg_F_leaves<Fr, 8, -1>), (tiles, a.n_gates), (threads), 0, st, a, lv, out, n0);
    else if (max_slots <= 16) SRS_LAUNCH((k_pg_F_leaves<Fr, 16, -1>), (tiles, a.n_gates), (threads), 0, st, a, lv, out, n0);
    else SRS_LAUNCH((k_pg_F_leaves<Fr, 32, -1>), (tiles, a.n_gates), (threads), 0, st, a, lv, out, n0);
}

// hoist (the reference's leaf rows): the gates at row 0 once, `row0_groups` workgroups per gate (hoist_mode 1), then the leaf pass reads
// them (hoist_mode 2).  Otherwise the leaf pass alone.
template <class Launch>
static void launch_hoisted(PgArgs &a, bool hoist, uint32_t row0_groups, uint32_t tiles, Launch &&leaves) {
    if (hoist) {
        a.hoist_mode = 1;
        leaves(row0_groups);
        a.hoist_mode = 2;
    }
    leaves(tiles);
}

// the inverse Vandermonde matrix [d + 1][d + 1] of the integer nodes first .. first + d, first = 0 | 1: coefficient k = sum_j M[k][j] value_j
static std::vector<fe_t> pg_node_matrix(const Structure *S, uint32_t d, uint32_t first) {
    FieldOps f{0};
    if (first) return !S->vinv_g1.empty() ? S->vinv_g1 : inverse_vandermonde_at(f, d, 1);
    const std::vector<fe_t> rows = !S->vinv_g.empty() ? S->vinv_g : (d ? inverse_vandermonde_rows(f, d) : std::vector<fe_t>());      // rows k = 1 .. d
    std::vector<fe_t> full((size_t)(d + 1) * (d + 1), Fr::zero());
    full[0] = Fr::one();                                       // coefficient 0 = the value at node 0
    std::copy(rows.begin(), rows.end(), full.begin() + (d + 1));
    return full;
}

// out[0 .. n_out): the coefficients of the polynomial of degree <= d_G with `values` at the nodes first_node .. first_node + d_G, then zeros
static void pg_interpolate(const Structure *S, const fe_t *values, uint32_t first_node, fe_t *out, size_t n_out) {
    const uint32_t n = (uint32_t)S->max_gate_degree + 1;
    const std::vector<fe_t> M = pg_node_matrix(S, n - 1, first_node);
    for (size_t k = 0; k < n_out; ++k) {
        fe_t acc = Fr::zero();
        for (uint32_t j = 0; j < n && k < n; ++j) acc = Fr::add(acc, Fr::mul(M[k * n + j], values[j]));
        out[k] = acc;
    }
}

// ---------------------------------------------------------------------------------------------
// The reference's leaf rows in closed form (reference_compat).  Every leaf of gate g is that gate AT ROW 0
// (src/plonk/mod.rs:714), one value c_g per (gate, point), and the weights are products over the index bits, pow_i(w) =
// prod_b w_b^bit_b(i), so the sum over gate g's aligned block of 2^k leaves factors:
//   sum_i pow_i(w) f_i = [prod_{b < k} (1 + w_b)] * sum_g c_g prod_{b >= k, bit_(b-k)(g) = 1} w_b        (padded blocks: no term)
// The device evaluates the gates at row 0 (pg_row0_values: one launch, one D2H of n_gates x points values); the sums are host
// arithmetic -- exact, hence the coefficients of the weighted trees bit for bit (those stay reachable: tuning pg_compat_tree).
// ---------------------------------------------------------------------------------------------
// evaluate_e and G at one point: c[g * stride], weights w[0 .. levels)
fe_t pg_closed_sum(const fe_t *c, size_t stride, uint32_t n_gates, uint32_t k, const fe_t *w, uint32_t levels) {
    fe_t acc = Fr::zero();
    for (uint32_t g = 0; g < n_gates; ++g) {
        fe_t t = c[(size_t)g * stride];
        for (uint32_t b = k; b < levels; ++b)
            if ((g >> (b - k)) & 1u) t = Fr::mul(t, w[b]);
        acc = Fr::add(acc, t);
    }
    for (uint32_t b = 0; b < k && b < levels; ++b) acc = Fr::mul(acc, Fr::add(Fr::one(), w[b]));
    return acc;
}

// compute_F: the same sum with the weights beta_b + X delta^(2^b), a product of linear polynomials: out[0 .. n_out), degree <= levels
void pg_closed_F(const fe_t *c, uint32_t n_gates, uint32_t k, const fe_t *betas, const fe_t &delta, uint32_t levels, fe_t *out, size_t n_out) {
    const std::vector<fe_t> deltas = pg_deltas(delta, levels);
    // p(X) *= (a + X d), deg = current degree
    auto mul_linear = [](std::vector<fe_t> &p, uint32_t &deg, const fe_t &a, const fe_t &d) {
        p[deg + 1] = Fr::mul(p[deg], d);
        for (uint32_t m = deg; m >= 1; --m) p[m] = Fr::add(Fr::mul(p[m], a), Fr::mul(p[m - 1], d));
        p[0] = Fr::mul(p[0], a);
        ++deg;
    };
    std::vector<fe_t> sum(levels + 2, Fr::zero()), t(levels + 2);
    for (uint32_t g = 0; g < n_gates; ++g) {
        std::fill(t.begin(), t.end(), Fr::zero());
        t[0] = c[g];
        uint32_t deg = 0;
        for (uint32_t b = k; b < levels; ++b)
            if ((g >> (b - k)) & 1u) mul_linear(t, deg, betas[b], deltas[b]);
        for (uint32_t m = 0; m <= deg; ++m) sum[m] = Fr::add(sum[m], t[m]);
    }
    uint32_t deg = levels > k ? levels - k : 0;
    for (uint32_t b = 0; b < k && b < levels; ++b) mul_linear(sum, deg, Fr::add(Fr::one(), betas[b]), deltas[b]);
    for (size_t m = 0; m < n_out; ++m) out[m] = m <= deg ? sum[m] : Fr::zero();
}

// compute_G from its gate values (PgRow0 of the folds): the point values by pg_closed_sum, then the interpolation of the route
// the values were taken on -- the constant inverse Vandermonde matrix of the integer nodes 0 .. d_G, or the inverse DFT over the
// P roots of unity (fft::ifft, :419; P <= 64 values: the plain sum on the host, no launch)
void pg_closed_G(const Structure *S, const PgRow0 &r0, const fe_t *betas_stroke, uint32_t levels, fe_t *out, size_t n_out, std::vector<fe_t> *point_values) {
    const uint32_t n_gates = (uint32_t)S->gate_progs.size(), P = r0.P;
    std::vector<fe_t> val(P);
    for (uint32_t p = 0; p < P; ++p) val[p] = pg_closed_sum(r0.vals.data() + p, P, n_gates, S->k, betas_stroke, levels);
    if (point_values) *point_values = val;
    if (r0.g_int) { pg_interpolate(S, val.data(), 0, out, n_out); return; }
    for (size_t m = 0; m < n_out; ++m) out[m] = Fr::zero();
    const fe_t winv = ntt::omega(ilog2(P), true), inv_P = Fr::inv(Fr::from_u64(P));
    fe_t wk = Fr::one();                                       // winv^k
    for (uint32_t k = 0; k < P && k < n_out; ++k) {
        fe_t acc = Fr::zero(), x = Fr::one();
        for (uint32_t p = 0; p < P; ++p) { acc = Fr::add(acc, Fr::mul(val[p], x)); x = Fr::mul(x, wk); }
        out[k] = Fr::mul(acc, inv_P);
        wk = Fr::mul(wk, winv);
    }
}

// The gates at row 0 in ONE launch, one workgroup per (point, gate) (the hoisting form of the leaf kernels), and one D2H.
// fold = false: on the trace W_dev[0] (compute_F, evaluate_e).  fold = true: on the fold of the J traces at each of compute_G's
// evaluation points -- the integers 0 .. d_G with one incoming trace, else the points_G roots of unity, the per-point challenges
// folded with L_j(X_p).  X = 1 is one of the points on both routes and the fold there IS W_dev[0]: out.one_at.
int pg_row0_values(Structure *S, bool fold, const fe_t *const *W_dev, const fe_t *const *challenges_host, size_t n_ch, size_t J, hipStream_t st,
                   PgRow0 &out, std::string &err) {
    if (S->field != 0) { err = "ProtoGalaxy polynomials need the 2-adic field bn256::Fr"; return 4; }
    if (J == 0 || J > JMAX) { err = "unsupported number of traces"; return 4; }
    PgSizes sz;
    if (!pg_sizes(S, fold ? J - 1 : 1, sz)) { err = "structure has no gates"; return 4; }
    const bool g_int = fold && J == 2 && tuning::get_or(tuning::PG_G_FFT, 0) == 0;
    const uint32_t P = !fold ? 1u : (g_int ? (uint32_t)S->max_gate_degree + 1 : (uint32_t)sz.points_G);
    const uint32_t n_gates = (uint32_t)S->gate_progs.size();
    out.P = P;
    out.g_int = g_int;
    out.one_at = g_int ? 1u : 0u;                              // integer nodes 0, 1, ..; roots of unity w^0 = 1, w, ..
    const PgPoints pp = pg_points(g_int, 0, P, fold, J, (uint32_t)sz.lagrange_domain, challenges_host, n_ch);
    // the specialised gate set in sweep form (k_pg_leaves_sweep<.., COMPAT>, hoist_mode 1) where the leaf route takes it, else the interpreter
    const bool sweep = S->pg_spec_id >= 0 && S->k >= 10 && (!fold || g_int) && P <= DMAX + 1;
    PgSlotWeights sw;
    sw.first = PG_LPT;
    sw.weighted = false;
    PgGateTable t;
    if (int rc = pg_gate_table(S, pp.ch_pt, n_ch, sweep ? &sw : nullptr, t, err)) return rc;
    Arena &A = S->arena;
    A.reserve(Arena::pad((pp.wcoef.size() + 1) * sizeof(fe_t)) + Arena::pad((t.utab.size() + 1) * sizeof(fe_t)) + Arena::pad(t.gp.size() * sizeof(GateProg)) +
              Arena::pad(((size_t)n_gates * P + 1) * sizeof(fe_t)) + 4096);
    A.reset();
    fe_t *d_coef = A.take<fe_t>(pp.wcoef.size() + 1);
    fe_t *d_utab = A.take<fe_t>(t.utab.size() + 1);
    GateProg *d_gp = A.take<GateProg>(t.gp.size());
    fe_t *d_vals = A.take<fe_t>((size_t)n_gates * P + 1);
    if (fold && !g_int) SRS_HIP_CHECK(hipMemcpyAsync(d_coef, pp.wcoef.data(), pp.wcoef.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemcpyAsync(d_utab, t.utab.data(), t.utab.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemcpyAsync(d_gp, t.gp.data(), t.gp.size() * sizeof(GateProg), hipMemcpyHostToDevice, st));
    PgCall c;
    c.n_w = J;
    c.J = (uint32_t)(fold ? J : 1);
    c.wcoef = (fold && !g_int) ? d_coef : nullptr;
    c.half = g_int ? 1u : 0u;
    c.leaf_pts = c.P = P;
    c.tile_log = S->k >= 10 ? 10u : std::min<uint32_t>(7, S->k);
    c.hoist = d_vals;
    PgArgs a = pg_args(S, W_dev, d_gp, d_utab, c);
    a.hoist_mode = 1;
    {
        prof::Scope ps("pg_row0", st, (size_t)n_gates * P);
        launch_leaves(S, a, P, (1u << a.tile_log) / (S->k >= 10 ? PG_LPT : 1u), sweep ? PG_LPT : 1u, t.max_slots, sweep, st);
    }
    out.vals.resize((size_t)n_gates * P);
    SRS_HIP_CHECK(hipMemcpyAsync(out.vals.data(), d_vals, out.vals.size() * sizeof(fe_t), hipMemcpyDeviceToHost, st));
    finish(st);
    return 0;
}

bool pg_closed_route(int compat) { return compat && tuning::get_or(tuning::PG_COMPAT_TREE, 0) == 0; }

// the reference's leaf rows: the gates at row 0 from the device, the sums in closed form on the host.  A row-sharded structure has
// nothing to shard here (every rank holds row 0): rank 0 returns the whole polynomial, the others the zero polynomial
static int pg_closed(Structure *S, int mode, const fe_t *const *W_dev, const fe_t *const *challenges_host, size_t n_ch, size_t J, const fe_t *weights_in,
                     const fe_t *delta, uint32_t levels, hipStream_t st, fe_t *out_host, uint32_t P_out, std::string &err) {
    for (uint32_t m = 0; m < P_out; ++m) out_host[m] = Fr::zero();
    if (S->shard_world > 1 && S->shard_rank != 0) return 0;
    PgRow0 r0;
    const int rc = pg_row0_values(S, mode == 1, W_dev, challenges_host, n_ch, J, st, r0, err);
    if (rc) return rc;
    const uint32_t n_gates = (uint32_t)S->gate_progs.size();
    if (mode == 0) pg_closed_F(r0.vals.data(), n_gates, S->k, weights_in, *delta, levels, out_host, P_out);
    else if (mode == 1) pg_closed_G(S, r0, weights_in, levels, out_host, P_out);
    else out_host[0] = pg_closed_sum(r0.vals.data(), 1, n_gates, S->k, weights_in, levels);
    return 0;
}

// compute_F with >= 1024 rows per gate: the polynomial tree (see k_pg_F_leaves).  The leaves carry F's coefficients of the three levels
// a thread reduces; the levels above multiply node polynomials by beta_b + X delta^(2^b).  -> out_host[0 .. P_out)
static int pg_F_tree(Structure *S, const fe_t *const *W_dev, const fe_t *const *challenges_host, size_t n_ch, const fe_t *betas, const fe_t &delta,
                     int compat, const PgSizes &sz, hipStream_t st, fe_t *out_host, uint32_t P_out, std::string &err) {
    const uint32_t levels = (uint32_t)sz.betas_count, n_gates = (uint32_t)S->gate_progs.size();
    const uint32_t tile_log = 10, TL = tile_log - 3, T = (1u << tile_log) / PG_LPT, tiles_per_gate = (uint32_t)(S->rows >> tile_log);
    const size_t n_tiles_valid = (size_t)n_gates * tiles_per_gate, n_tiles_padded = sz.count_with_padding >> tile_log;
    const PgPoints pp = pg_points(false, 0, 1, false, 1, 0, challenges_host, n_ch);
    PgGateTable t;
    if (int rc = pg_gate_table(S, pp.ch_pt, n_ch, nullptr, t, err)) return rc;
    const size_t n0 = n_tiles_padded * T;
    Arena &A = S->arena;
    A.reserve(2 * Arena::pad((4 * n0 + 64) * sizeof(fe_t)) + Arena::pad((t.utab.size() + 1) * sizeof(fe_t)) +
              Arena::pad(t.gp.size() * sizeof(GateProg)) + Arena::pad((n_gates + 1) * sizeof(fe_t)) + 4096);
    A.reset();
    fe_t *d_utab = A.take<fe_t>(t.utab.size() + 1);
    GateProg *d_gp = A.take<GateProg>(t.gp.size());
    fe_t *cur = A.take<fe_t>(4 * n0 + 64), *nxt = A.take<fe_t>(4 * n0 + 64);
    fe_t *d_hoist = A.take<fe_t>(n_gates + 1);
    SRS_HIP_CHECK(hipMemcpyAsync(d_utab, t.utab.data(), t.utab.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemcpyAsync(d_gp, t.gp.data(), t.gp.size() * sizeof(GateProg), hipMemcpyHostToDevice, st));
    const std::vector<fe_t> deltas = pg_deltas(delta, levels);
    PgCall c;
    c.compat = compat;
    c.tile_log = tile_log;
    c.sharded = true;
    c.hoist = d_hoist;
    PgArgs a = pg_args(S, W_dev, d_gp, d_utab, c);
    PgFLevels lv;
    for (uint32_t j = 0; j < 3; ++j) { lv.beta[j] = betas[TL + j]; lv.delta[j] = deltas[TL + j]; }
    {
        prof::Scope ps("pg_F_leaves", st, S->rows * n_gates);
        // the reference's leaf rows: the gates at row 0 once, then the leaf pass reads them
        launch_hoisted(a, compat != 0, 1, tiles_per_gate, [&](uint32_t tiles) { launch_F_leaves(S, a, lv, tiles, T, t.max_slots, cur, (uint32_t)n0, st); });
    }
    // remaining leaf-index bits, in the order adjacent nodes differ: thread bits 0 .. TL-1, then tile / gate bits TL+3 ..
    std::vector<uint32_t> order;
    for (uint32_t b = 0; b < TL; ++b) order.push_back(b);
    for (uint32_t b = TL + 3; b < levels; ++b) order.push_back(b);
    size_t n_in = n0, m_valid = n_tiles_valid * T;
    uint32_t deg = 3;
    size_t at = 0;
    // (dynamic LDS of a launch stays below 48 KiB: degree <= 23 after the launch -- every table size an NTT of <= 2^28 allows; beyond, the r03 flow)
    while (at < order.size() && deg + std::min<size_t>(PG_F_MULTI_LEVELS, order.size() - at) <= 23) {
        // up to six levels per launch (k_pg_F_multi); what is left beyond degree 23: one launch per level + the one-workgroup tail
        const uint32_t nlev = (uint32_t)std::min<size_t>(PG_F_MULTI_LEVELS, order.size() - at);
        PgFMulti tm;
        for (uint32_t l = 0; l < PG_F_MULTI_LEVELS; ++l) {
            tm.beta[l] = l < nlev ? betas[order[at + l]] : Fr::zero();
            tm.delta[l] = l < nlev ? deltas[order[at + l]] : Fr::zero();
        }
        const size_t n_out = n_in >> nlev;
        const size_t lds = 2 * (size_t)PG_F_MULTI_NODES * (deg + nlev + 1) * sizeof(fe_t);
        SRS_LAUNCH((k_pg_F_multi<Fr>), ((uint32_t)n_out), (256), lds, st, (const fe_t *)cur, (uint32_t)n_in, (uint32_t)m_valid, deg, nlev, tm, nxt,
                   (uint32_t)n_out);
        n_in = n_out;
        m_valid = (m_valid + (((size_t)1 << nlev) - 1)) >> nlev;
        deg += nlev;
        at += nlev;
        std::swap(cur, nxt);
    }
    for (; at < order.size(); ++at) {
        // the last levels (<= 32 nodes left) run in one workgroup (k_pg_F_tail)
        const size_t left = order.size() - at;
        if (n_in <= 32 && left <= PG_F_TAIL_LEVELS && deg + left <= PG_F_TAIL_MAXDEG) break;
        const uint32_t b = order[at];
        const size_t n_out = n_in / 2;
        SRS_LAUNCH((k_pg_F_level<Fr>), ((uint32_t)((n_out * (deg + 2) + 127) / 128)), (128), 0, st, (const fe_t *)cur, (uint32_t)n_in,
                   (uint32_t)m_valid, deg, betas[b], deltas[b], nxt, (uint32_t)n_out);
        n_in = n_out;
        m_valid = (m_valid + 1) / 2;
        ++deg;
        std::swap(cur, nxt);
    }
    if (at < order.size()) {
        const uint32_t nlev = (uint32_t)(order.size() - at);
        PgFTail tl;
        for (uint32_t l = 0; l < PG_F_TAIL_LEVELS; ++l) {
            tl.beta[l] = l < nlev ? betas[order[at + l]] : Fr::zero();
            tl.delta[l] = l < nlev ? deltas[order[at + l]] : Fr::zero();
        }
        SRS_LAUNCH((k_pg_F_tail<Fr>), (1), (512), 0, st, (const fe_t *)cur, (uint32_t)n_in, (uint32_t)m_valid, deg, nlev, tl, nxt);
        deg += nlev;
        std::swap(cur, nxt);
    }
    // n_in == 1: cur[m] = coefficient m, m <= deg = levels; the reference's vector has fft_points_count_F entries
    std::vector<fe_t> coef(deg + 1);
    SRS_HIP_CHECK(hipMemcpyAsync(coef.data(), cur, coef.size() * sizeof(fe_t), hipMemcpyDeviceToHost, st));
    finish(st);
    for (uint32_t m = 0; m < P_out; ++m) out_host[m] = m < coef.size() ? coef[m] : Fr::zero();
    return 0;
}

// the upper levels of the weighted tree over the tile partials in `cur` (m of them, zero padding beyond the m_valid of the real gates)
// -> the device pointer of the P sums (`cur` or `nxt`)
static fe_t *pg_reduce(fe_t *cur, fe_t *nxt, size_t m, size_t m_valid, uint32_t P, const fe_t *d_w, uint32_t wpts, uint32_t level0, hipStream_t st) {
    while (m > 1) {
        uint32_t lv = std::min<uint32_t>(7, ilog2(m));
        uint32_t outs = (uint32_t)(m >> lv);
        if (((size_t)P << lv) <= PG_REDUCE_PAR_THREADS && (((size_t)P << lv) % 64 == 0 || outs == 1))
            SRS_LAUNCH((k_pg_reduce_par<Fr>), (outs), (1u << lv, P), 0, st, (const fe_t *)cur, (uint32_t)m_valid, P, d_w, wpts, level0, lv, nxt);
        else
            SRS_LAUNCH((k_pg_reduce<Fr>), (outs), (1u << lv), 0, st, (const fe_t *)cur, (uint32_t)m_valid, P, d_w, wpts, level0, lv, nxt);
        level0 += lv;
        m = outs;
        m_valid = outs;
        std::swap(cur, nxt);
    }
    return cur;
}

// Leaves + weighted reduce: compute_G, evaluate_e, and compute_F on small tables or as the cross-check of the tree (tuning pg_f_eval = 1).
// One leaf launch leaves a partial sum per (tile, point), pg_reduce the P sums; then G / F are interpolated from them.
static int pg_leaf_sums(Structure *S, int mode, const fe_t *const *W_dev, const fe_t *const *challenges_host, size_t n_ch, size_t J, const fe_t *weights_in,
                        const fe_t *delta, int compat, const PgSizes &sz, hipStream_t st, fe_t *out_host, uint32_t P_out, size_t *n_out, std::string &err,
                        const fe_t *g_at_one, PgGValues *keep_on_device) {
    // compute_G with one incoming trace (L = 1, Lagrange domain {1, -1}): the folded witness L_0(X) w_0 + L_1(X) w_1 =
    // (w_0 + w_1)/2 + X (w_0 - w_1)/2 is LINEAR in X, so G has degree <= max gate degree d_G.  Instead of the reference's
    // next_pow2(d_G + 1) roots of unity (2 multiplies per advice load to fold the witness, then an ifft) G is evaluated at
    // the integers 0..d_G (fold = halvings + additions, d_G + 1 points) and interpolated with the constant inverse
    // Vandermonde matrix: the same polynomial, hence the same coefficients (exact arithmetic), ~35 % less work.
    const bool g_int = mode == 1 && J == 2 && tuning::get_or(tuning::PG_G_FFT, 0) == 0;      // (tuning pg_g_fft: the L >= 2 route on L = 1, for the equality test)
    const uint32_t dG = (uint32_t)S->max_gate_degree;
    // 8 leaves per thread once a gate has >= 1024 rows: 1024-leaf tiles, the first three tree levels in registers
    const uint32_t lpt = S->k >= 10 ? PG_LPT : 1u;
    const uint32_t tile_log = lpt == PG_LPT ? 10u : std::min<uint32_t>(7, S->k);
    // ... and one of the d_G + 1 values is free for a caller that has F: at X = 1 the fold IS the accumulator (L_0(1) = 1), the
    // weights are betas_stroke = beta + alpha delta^(2^b), so G(1) = sum_i pow_i(betas_stroke) f_i(acc) = F(alpha) -- an
    // identity of the definitions, whatever the traces hold.  ProtoGalaxy::prove has F(alpha) (it is compute_K's first
    // argument): with `g_at_one` the leaves are evaluated at X = 2 .. d_G + 1 only (d_G points), and the interpolation
    // nodes are 1 .. d_G + 1.  Needs a sweep-form leaf kernel (below; ahead of time or compiled); otherwise all d_G + 1 points are evaluated.
    const bool skip_one = g_int && g_at_one != nullptr && dG >= 2 && pg_leaf_sweep_form(S, compat) && lpt == PG_LPT && dG + 1 <= DMAX + 1;
    const uint32_t pt0 = skip_one ? 2u : 0u;
    const uint32_t P = g_int ? (skip_one ? dG : dG + 1) : P_out;   // evaluation points actually used
    const uint32_t leaf_pts = mode == 1 ? P : 1u;
    const uint32_t wpts = mode == 0 ? P : 1u;
    const uint32_t levels = (uint32_t)sz.betas_count, n_gates = (uint32_t)S->gate_progs.size();
    const PgPoints pp = pg_points(g_int, pt0, P, mode == 1, J, (uint32_t)sz.lagrange_domain, challenges_host, n_ch);
    // ---- weights [levels][wpts]: F's are beta_b + X_p delta^(2^b)  (:102-111)
    std::vector<fe_t> weights(weights_in, weights_in + levels);
    if (mode == 0) {
        const std::vector<fe_t> deltas = pg_deltas(*delta, levels);
        weights.resize((size_t)levels * P);
        for (uint32_t b = 0; b < levels; ++b)
            for (uint32_t p = 0; p < P; ++p) weights[(size_t)b * P + p] = Fr::add(weights_in[b], Fr::mul(pp.pts[p], deltas[b]));
    }
    // the specialised leaf kernel in sweep form (k_pg_leaves_sweep, or its run-time compiled twin): integer-point G and evaluate_e
    const bool sweep_leaves = pg_leaf_sweep_form(S, compat) && lpt == PG_LPT && mode != 0 && (mode != 1 || g_int) && P <= DMAX + 1;
    PgSlotWeights sw;
    if (sweep_leaves) sw = pg_slot_weights_leaves(weights.data() + (tile_log - 3));      // (wpts == 1 in sweep form)
    PgGateTable t;
    if (int rc = pg_gate_table(S, pp.ch_pt, n_ch, sweep_leaves ? &sw : nullptr, t, err)) return rc;
    const uint32_t tile = (1u << tile_log) / lpt, tiles_per_gate = (uint32_t)(S->rows >> tile_log);
    const size_t n_tiles_valid = (size_t)n_gates * tiles_per_gate, n_tiles_padded = sz.count_with_padding >> tile_log;
    // ---- device staging
    Arena &A = S->arena;
    A.reserve(Arena::pad(weights.size() * sizeof(fe_t)) + Arena::pad((pp.wcoef.size() + 1) * sizeof(fe_t)) +
              Arena::pad((t.utab.size() + 1) * sizeof(fe_t)) + Arena::pad(t.gp.size() * sizeof(GateProg)) +
              2 * Arena::pad((n_tiles_padded + 1) * P * sizeof(fe_t)) + Arena::pad(sizeof(fe_t) * P) +
              Arena::pad(((size_t)n_gates * P + 1) * sizeof(fe_t)) + 4096);
    A.reset();
    fe_t *d_w = A.take<fe_t>(weights.size());
    fe_t *d_coef = A.take<fe_t>(pp.wcoef.size() + 1);
    fe_t *d_utab = A.take<fe_t>(t.utab.size() + 1);
    GateProg *d_gp = A.take<GateProg>(t.gp.size());
    fe_t *buf0 = A.take<fe_t>((n_tiles_padded + 1) * P);
    fe_t *buf1 = A.take<fe_t>((n_tiles_padded + 1) * P);
    fe_t *d_hoist = A.take<fe_t>((size_t)n_gates * P + 1);
    SRS_HIP_CHECK(hipMemcpyAsync(d_w, weights.data(), weights.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    if (!pp.wcoef.empty()) SRS_HIP_CHECK(hipMemcpyAsync(d_coef, pp.wcoef.data(), pp.wcoef.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemcpyAsync(d_utab, t.utab.data(), t.utab.size() * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemcpyAsync(d_gp, t.gp.data(), t.gp.size() * sizeof(GateProg), hipMemcpyHostToDevice, st));
    PgCall c;
    c.n_w = J;
    c.J = (uint32_t)(mode == 1 ? J : 1);
    c.wcoef = (mode == 1 && !g_int) ? d_coef : nullptr;
    c.half = g_int ? 1u : 0u;
    c.pt0 = pt0;
    c.compat = compat;
    c.leaf_pts = leaf_pts;
    c.P = P;
    c.wpts = wpts;
    c.tile_log = tile_log;
    c.weights = d_w;
    c.partial = buf0;
    c.hoist = d_hoist;
    c.sharded = true;
    PgArgs a = pg_args(S, W_dev, d_gp, d_utab, c);
    {
        prof::Scope ps(mode == 0 ? "pg_F_leaves" : (mode == 1 ? "pg_G_leaves" : "pg_e_leaves"), st, S->rows * n_gates);
        // the reference's leaf rows: the gates at row 0 once per (gate, point) -- the interpreter and the sweep form; the plain ahead-of-time
        // kernel evaluates per thread -- then the leaf pass runs the weighted trees
        const bool hoist = compat && (sweep_leaves || !(S->pg_spec_id >= 0 && lpt == PG_LPT));
        launch_hoisted(a, hoist, leaf_pts, tiles_per_gate, [&](uint32_t tiles) { launch_leaves(S, a, tiles, tile, lpt, t.max_slots, sweep_leaves, st); });
    }
    fe_t *sums = pg_reduce(buf0, buf1, n_tiles_padded, n_tiles_valid, P, d_w, wpts, tile_log, st);
    if (g_int && keep_on_device && dG + 1 <= PG_K_SMALL_MAX_NODES) {      // the caller goes on to K on the device (pg_K_from_G_device): no round trip through the host here
        keep_on_device->vals_dev = sums;
        keep_on_device->n_dev = P;
        keep_on_device->degree = dG;
        keep_on_device->skip_one = skip_one;
        *n_out = 0;
        return 0;
    }
    *n_out = P_out;
    if (g_int) {
        // G at the nodes 0 .. dG, or 1 .. dG + 1 with G(1) = F(alpha) in front of the evaluated ones
        std::vector<fe_t> val(dG + 1);
        if (skip_one) val[0] = *g_at_one;
        SRS_HIP_CHECK(hipMemcpyAsync(val.data() + (skip_one ? 1 : 0), sums, (size_t)P * sizeof(fe_t), hipMemcpyDeviceToHost, st));
        finish(st);
        pg_interpolate(S, val.data(), skip_one ? 1 : 0, out_host, P_out);
        return 0;
    }
    if (mode != 2 && P > 1) ntt::run(sums, ilog2(P), P, 1, true, false, st);      // fft::ifft(&mut points)  (:197, :419)
    SRS_HIP_CHECK(hipMemcpyAsync(out_host, sums, (size_t)P * sizeof(fe_t), hipMemcpyDeviceToHost, st));
    finish(st);
    return 0;
}

// mode 0: compute_F, 1: compute_G, 2: evaluate_e.  W_dev: J device witness pointers (J = 1 for F / e).
// challenges_host: J arrays of n_ch challenges.  weights_in: betas (F, e) / betas_stroke (G), betas_count values.
// out_host: points_F / points_G coefficients (after ifft) or the single value e.
int pg_sum(Structure *S, int mode, const fe_t *const *W_dev, const fe_t *const *challenges_host, size_t n_ch, size_t J,
           const fe_t *weights_in, size_t n_weights, const fe_t *delta, int compat, hipStream_t st, fe_t *out_host,
           size_t *n_out, std::string &err, const fe_t *g_at_one, PgGValues *keep_on_device) {
    if (S->field != 0) { err = "ProtoGalaxy polynomials need the 2-adic field bn256::Fr"; return 4; }
    if (J == 0 || J > JMAX) { err = "unsupported number of traces"; return 4; }
    PgSizes sz;
    if (!pg_sizes(S, mode == 1 ? J - 1 : 1, sz)) { *n_out = 0; return 0; }
    if (n_weights < sz.betas_count) { err = "not enough betas"; return 4; }
    const uint32_t P_out = mode == 0 ? (uint32_t)sz.points_F : (mode == 1 ? (uint32_t)sz.points_G : 1u);
    if (pg_closed_route(compat)) {
        *n_out = P_out;
        return pg_closed(S, mode, W_dev, challenges_host, n_ch, J, weights_in, delta, (uint32_t)sz.betas_count, st, out_host, P_out, err);
    }
    // leaves over rows from here on.  The intended rows of a gate set without ahead-of-time kernels: compile its leaf kernels on the first
    // such call (never at creation: the reference's rows above pay nothing); whatever excludes it or fails leaves the interpreter in place
    if (!compat) { std::string why; (void)pg_jit_ensure(S, true, nullptr, why); }
    // the evaluate-and-interpolate route of compute_F stays for small tables and as the cross-check (tuning pg_f_eval = 1)
    if (mode == 0 && S->k >= 10 && tuning::get_or(tuning::PG_F_EVAL, 0) == 0) {
        *n_out = P_out;
        return pg_F_tree(S, W_dev, challenges_host, n_ch, weights_in, *delta, compat, sz, st, out_host, P_out, err);
    }
    return pg_leaf_sums(S, mode, W_dev, challenges_host, n_ch, J, weights_in, delta, compat, sz, st, out_host, P_out, n_out, err, g_at_one, keep_on_device);
}

// compute_K_from_G's small domain (256 points in every configuration, quirk Q2).  Everything that depends on the domain only -- the points
// X_i = zeta omega^i, L_0(X_i) = Z(X_i) / (n (X_i - 1)) (lagrange.rs:50-75) and 1 / Z(X_i) -- is computed once per (domain, n) with ONE inversion
// for all denominators (Montgomery's trick) and kept: tab = [xs | l0 | inv_z], count each.  zero_z: some Z(X_i) = 0, no l0 / inv_z
struct KDomain { std::vector<fe_t> tab; bool zero_z = false; };
static const KDomain &k_domain_table(uint32_t log_domain_K, size_t instances_to_fold) {
    static std::mutex mu;
    static std::map<std::pair<uint32_t, size_t>, KDomain> cache;
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find({log_domain_K, instances_to_fold});
    if (it != cache.end()) return it->second;
    const size_t count = (size_t)1 << log_domain_K;
    KDomain d;
    const fe_t zeta = ntt::zeta(), omega = ntt::omega(log_domain_K, false), one = Fr::one();
    const fe_t inv_n = Fr::inv(Fr::from_u64(instances_to_fold));
    d.tab.resize(3 * count);
    fe_t *xs = d.tab.data(), *l0 = xs + count, *inv_z = l0 + count;
    std::vector<fe_t> xn1(count), xm1(count), pref(2 * count);
    fe_t X = zeta, acc = one;
    for (size_t i = 0; i < count; ++i) { xs[i] = X; X = Fr::mul(X, omega); }
    for (size_t i = 0; i < count; ++i) {
        xn1[i] = Fr::sub(Fr::pow_u64(xs[i], instances_to_fold), one);
        xm1[i] = Fr::sub(xs[i], one);
        if (Fr::is_zero(xn1[i])) d.zero_z = true;                                  // X = 1 included (then X - 1 = 0 too)
    }
    if (!d.zero_z) {
        for (size_t i = 0; i < count; ++i) {
            pref[2 * i] = acc;
            acc = Fr::mul(acc, xn1[i]);
            pref[2 * i + 1] = acc;
            acc = Fr::mul(acc, xm1[i]);
        }
        fe_t inv = Fr::inv(acc);
        for (size_t i = count; i-- > 0;) {
            const fe_t inv_xm1 = Fr::mul(inv, pref[2 * i + 1]);
            inv = Fr::mul(inv, xm1[i]);
            inv_z[i] = Fr::mul(inv, pref[2 * i]);
            inv = Fr::mul(inv, xn1[i]);
            l0[i] = Fr::mul(inv_n, Fr::mul(xn1[i], inv_xm1));
        }
    }
    return cache.emplace(std::make_pair(log_domain_K, instances_to_fold), std::move(d)).first->second;      // (map nodes do not move)
}

// compute_K_from_G (src/nifs/protogalaxy/poly/mod.rs:475-509)
int pg_K_from_G(const fe_t *polyG_host, size_t nG, const fe_t &f_alpha, size_t instances_to_fold, uint32_t log_domain_K,
                hipStream_t st, fe_t *out_host, std::string &err) {
    if (log_domain_K > ntt::FR_S) { err = "k=" + std::to_string(log_domain_K) + " should no larger than F::S=28"; return 3; }   // fft.rs:13
    const size_t count = (size_t)1 << log_domain_K;
    static thread_local ThreadArena scratch;                         // grow-only: no hipMalloc / hipFree (implicit sync) per call
    scratch.reserve(Arena::pad((nG + 1) * sizeof(fe_t)) + Arena::pad(count * sizeof(fe_t)) + Arena::pad(sizeof(int)) + 256);
    scratch.reset();
    fe_t *d_g = scratch.take<fe_t>(nG + 1), *d_out = scratch.take<fe_t>(count);
    int *d_err = scratch.take<int>(1);
    int herr = 0;
    if (count <= 4096) {
        // The K domain is tiny: the points are computed on the host from the kept table.  A GPU thread per point spends two Fermat
        // inversions = 760 dependent multiplications = 0.6 ms of pure latency on it.
        const KDomain &dom = k_domain_table(log_domain_K, instances_to_fold);
        if (dom.zero_z) { err = "Z(X) must be not equal to 0"; return 4; }
        const fe_t *xs = dom.tab.data(), *l0 = xs + count, *inv_z = l0 + count;
        std::vector<fe_t> kp(count);
        // 256 x (nG Horner steps + 2 products) = ~3 k field products = ~0.1 ms on one core: less than starting helper threads
        // costs (the r01 / early r02 version spawned 8 std::threads per call: 0.2 ms of the gap after compute_G)
        for (size_t i = 0; i < count; ++i) {
            fe_t gi = Fr::zero();
            for (size_t k = nG; k-- > 0;) gi = Fr::add(Fr::mul(gi, xs[i]), polyG_host[k]);   // UnivariatePoly::eval (univariate.rs:67-75), Horner: same value
            kp[i] = Fr::mul(Fr::sub(gi, Fr::mul(f_alpha, l0[i])), inv_z[i]);
        }
        SRS_HIP_CHECK(hipMemcpyAsync(d_out, kp.data(), count * sizeof(fe_t), hipMemcpyHostToDevice, st));
        ntt::run(d_out, log_domain_K, count, 1, true, true, st);     // UnivariatePoly::coset_ifft
        SRS_HIP_CHECK(hipMemcpyAsync(out_host, d_out, count * sizeof(fe_t), hipMemcpyDeviceToHost, st));
        SRS_HIP_CHECK(hipStreamSynchronize(st));
        return 0;
    }
    SRS_HIP_CHECK(hipMemcpyAsync(d_g, polyG_host, nG * sizeof(fe_t), hipMemcpyHostToDevice, st));
    SRS_HIP_CHECK(hipMemsetAsync(d_err, 0, sizeof(int), st));
    fe_t inv_n = Fr::inv(Fr::from_u64(instances_to_fold));
    SRS_LAUNCH(k_pg_K_points, ((uint32_t)((count + 63) / 64)), (64), 0, st, (const fe_t *)d_g, (uint32_t)nG, f_alpha,
               ntt::zeta(), ntt::omega(log_domain_K, false), inv_n, (uint32_t)instances_to_fold, (uint32_t)count, d_out, d_err);
    ntt::run(d_out, log_domain_K, count, 1, true, true, st);     // UnivariatePoly::coset_ifft
    SRS_HIP_CHECK(hipMemcpyAsync(out_host, d_out, count * sizeof(fe_t), hipMemcpyDeviceToHost, st));
    SRS_HIP_CHECK(hipMemcpyAsync(&herr, d_err, sizeof(int), hipMemcpyDeviceToHost, st));
    SRS_HIP_CHECK(hipStreamSynchronize(st));
    if (herr) { err = "Z(X) must be not equal to 0"; return 4; }
    return 0;
}

// the host's table of the small K domain on the device, per (domain, n, device); nullptr with zero_z
static const fe_t *k_domain_table_dev(uint32_t log_domain_K, size_t instances_to_fold, bool &zero_z) {
    static std::mutex mu;
    static std::map<std::tuple<int, uint32_t, size_t>, fe_t *> cache;
    const KDomain &dom = k_domain_table(log_domain_K, instances_to_fold);
    zero_z = dom.zero_z;
    if (zero_z) return nullptr;
    int device = 0;
    SRS_HIP_CHECK(hipGetDevice(&device));
    std::lock_guard<std::mutex> lk(mu);
    fe_t *&dev = cache[std::make_tuple(device, log_domain_K, instances_to_fold)];
    if (!dev) {
        fe_t *d = nullptr;
        SRS_HIP_CHECK(hipMalloc((void **)&d, dom.tab.size() * sizeof(fe_t)));        // kept for the life of the process (24 KiB per domain)
        SRS_HIP_CHECK(hipMemcpy(d, dom.tab.data(), dom.tab.size() * sizeof(fe_t), hipMemcpyHostToDevice));
        dev = d;
    }
    return dev;
}

bool pg_K_device_ok(const PgGValues &g, uint32_t log_domain_K) {
    return g.vals_dev != nullptr && g.degree + 1 <= PG_K_SMALL_MAX_NODES && log_domain_K <= PG_K_SMALL_MAX_LOG;
}

int pg_K_from_G_device(Structure *S, const PgGValues &g, const fe_t &f_alpha, size_t instances_to_fold, uint32_t log_domain_K, hipStream_t st,
                       fe_t *out_host, std::string &err) {
    if (!pg_K_device_ok(g, log_domain_K)) { err = "internal: pg_K_from_G_device on an unsupported shape"; return 5; }
    const uint32_t n_nodes = g.degree + 1, count = 1u << log_domain_K;
    bool zero_z = false;
    const fe_t *tab = k_domain_table_dev(log_domain_K, instances_to_fold, zero_z);
    if (zero_z) { err = "Z(X) must be not equal to 0"; return 4; }
    fe_t *&M = S->d_kM[g.skip_one ? 1 : 0];
    if (!M) {
        const std::vector<fe_t> full = pg_node_matrix(S, g.degree, g.skip_one ? 1 : 0);
        SRS_HIP_CHECK(hipMalloc((void **)&M, full.size() * sizeof(fe_t)));
        S->owned.push_back(M);
        SRS_HIP_CHECK(hipMemcpy(M, full.data(), full.size() * sizeof(fe_t), hipMemcpyHostToDevice));
    }
    static thread_local ThreadArena scratch;
    scratch.reserve(Arena::pad((size_t)count * sizeof(fe_t)) + 256);
    scratch.reset();
    fe_t *d_out = scratch.take<fe_t>(count);
    const uint32_t threads = std::max<uint32_t>(64u, std::min<uint32_t>(256u, count));
    SRS_LAUNCH(k_pg_K_small, ((count + threads - 1) / threads), (threads), 0, st, g.vals_dev, g.n_dev, f_alpha, g.skip_one ? 1 : 0, (const fe_t *)M,
               n_nodes, f_alpha, tab, count, d_out);
    ntt::run(d_out, log_domain_K, count, 1, true, true, st);     // UnivariatePoly::coset_ifft
    SRS_HIP_CHECK(hipMemcpyAsync(out_host, d_out, (size_t)count * sizeof(fe_t), hipMemcpyDeviceToHost, st));
    finish(st);
    return 0;
}

// the same from HOST values of G at the integer nodes 0 .. n - 1 (the closed-form compute_G): one small H2D in front
int pg_K_from_G_values(Structure *S, const fe_t *vals_host, uint32_t n, const fe_t &f_alpha, size_t instances_to_fold, uint32_t log_domain_K,
                       hipStream_t st, fe_t *out_host, std::string &err) {
    static thread_local ThreadArena scratch;
    scratch.reserve(Arena::pad((size_t)n * sizeof(fe_t)) + 256);
    scratch.reset();
    fe_t *d_vals = scratch.take<fe_t>(n);
    SRS_HIP_CHECK(hipMemcpyAsync(d_vals, vals_host, (size_t)n * sizeof(fe_t), hipMemcpyHostToDevice, st));
    PgGValues g;
    g.vals_dev = d_vals;
    g.n_dev = n;
    g.degree = n - 1;
    g.skip_one = false;
    return pg_K_from_G_device(S, g, f_alpha, instances_to_fold, log_domain_K, st, out_host, err);     // synchronises: vals_host may go
}

size_t count_mismatch(const fe_t *a_dev, const fe_t *b_dev, size_t n, hipStream_t st) {
    if (!n) return 0;
    uint32_t *d = nullptr, h = 0;
    SRS_HIP_CHECK(hipMalloc((void **)&d, sizeof(uint32_t)));
    SRS_HIP_CHECK(hipMemsetAsync(d, 0, sizeof(uint32_t), st));
    SRS_LAUNCH(k_count_mismatch, ((uint32_t)((n + 255) / 256)), (256), 0, st, a_dev, b_dev, n, d);
    SRS_HIP_CHECK(hipMemcpyAsync(&h, d, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    SRS_HIP_CHECK(hipStreamSynchronize(st));
    (void)hipFree(d);
    return h;
}

// ---------------------------------------------------------------------------------------------
// lookup arguments: host side
// ---------------------------------------------------------------------------------------------
// Arguments::evaluate_coefficient_1 (src/plonk/lookup.rs:319-341): ls[i] = L_i(row), ts[i] = T_i(row), ms[i].
// advice_dev: the advice columns, column-major num_advice * rows; outputs: HOST arrays of L DEVICE vectors.
int lookup_coeff_1(Structure *S, const fe_t *advice_dev, const fe_t &r, fe_t *const *ls, fe_t *const *ts, fe_t *const *ms,
                   hipStream_t st, std::string &err) {
    const size_t L = S->num_lookups;
    if (!L) { err = "structure has no lookup arguments"; return 4; }    // SpsError::LackOfLookupArguments
    const uint32_t n = (uint32_t)S->rows;
    for (size_t i = 0; i < 2 * L; ++i) {
        fe_t *outs[1] = {i < L ? ls[i] : ts[i - L]};
        int rc = evaluate_prog(S, S->lookup_progs[i], 1, advice_dev, nullptr, &r, 1, outs, st, err);
        if (rc) return rc;
    }
    uint32_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    uint32_t *d_row = nullptr, *d_cnt = nullptr;
    SRS_HIP_CHECK(hipMalloc((void **)&d_row, (size_t)cap * 2 * sizeof(uint32_t)));
    d_cnt = d_row + cap;
    try {
        const uint32_t blocks = (n + 255) / 256;
        for (size_t i = 0; i < L; ++i) {
            prof::Scope ps("lookup_m", st, n);
            SRS_HIP_CHECK(hipMemsetAsync(d_row, 0, (size_t)cap * 2 * sizeof(uint32_t), st));      // rows (M_EMPTY) and counts
            SRS_LAUNCH(k_m_insert, (blocks), (256), 0, st, (const fe_t *)ts[i], n, d_row, cap - 1);
            SRS_LAUNCH(k_m_count, (blocks), (256), 0, st, (const fe_t *)ls[i], n, (const fe_t *)ts[i], (const uint32_t *)d_row, d_cnt, cap - 1);
            if (S->field == 0) SRS_LAUNCH((k_m_emit<Fr>), (blocks), (256), 0, st, (const fe_t *)ts[i], n, (const uint32_t *)d_row, (const uint32_t *)d_cnt, cap - 1, ms[i]);
            else SRS_LAUNCH((k_m_emit<Fq>), (blocks), (256), 0, st, (const fe_t *)ts[i], n, (const uint32_t *)d_row, (const uint32_t *)d_cnt, cap - 1, ms[i]);
        }
        SRS_HIP_CHECK(hipStreamSynchronize(st));
        SRS_HIP_CHECK(hipGetLastError());
    } catch (...) { (void)hipFree(d_row); throw; }
    (void)hipFree(d_row);
    prof::collect();
    return 0;
}

// run_sps_protocol_2 / _3 (src/plonk/mod.rs:503-662) on the witness IN PLACE: W_dev = advice | ls | ts | ms | hs | gs, every group
// num_lookups columns of `rows` elements (the reference's concat_vec! grouping).  Both rounds only enqueue on `st` -- no allocation and
// no synchronisation once the structure's scratch has grown to its size; the caller's commit of the round is what waits.
// Round 1, evaluate_coefficient_1 (lookup.rs:319-341): the 2 L lookup / table programs write l_i, t_i to their places, then ONE
// multiplicity pass for all lookups -- one clear, three launches with the lookup in blockIdx.y -- writes m_i.
int sps_lookup_round_1(Structure *S, fe_t *W_dev, const fe_t &r, hipStream_t st, std::string &err) {
    const size_t L = S->num_lookups;
    if (!L) { err = "structure has no lookup arguments"; return 4; }    // SpsError::LackOfLookupArguments
    if (L > 65535) { err = "more than 65535 lookup arguments"; return 4; }      // gridDim.y / .z
    const uint32_t n = (uint32_t)S->rows;
    fe_t *ls = W_dev + S->num_advice * S->rows, *ts = ls + L * S->rows, *ms = ts + L * S->rows;
    for (size_t i = 0; i < 2 * L; ++i) {
        fe_t *outs[1] = {ls + i * S->rows};
        int rc = evaluate_prog(S, S->lookup_progs[i], 1, W_dev, nullptr, &r, 1, outs, st, err, false);
        if (rc) return rc;
    }
    uint32_t cap = 2;
    while (cap < 2 * n) cap <<= 1;
    const size_t words = 2 * L * (size_t)cap;                 // [L][cap] rows, then [L][cap] counts
    S->lookup_scratch.reserve(Arena::pad(words * sizeof(uint32_t)));
    S->lookup_scratch.reset();
    uint32_t *d_row = S->lookup_scratch.take<uint32_t>(words), *d_cnt = d_row + L * (size_t)cap;
    const uint32_t blocks = (n + 255) / 256, gy = (uint32_t)L;
    prof::Scope ps("lookup_m", st, n * L);
    SRS_HIP_CHECK(hipMemsetAsync(d_row, 0, words * sizeof(uint32_t), st));
    SRS_LAUNCH(k_m_insert, (blocks, gy), (256), 0, st, (const fe_t *)ts, n, d_row, cap - 1);
    SRS_LAUNCH(k_m_count, (blocks, gy), (256), 0, st, (const fe_t *)ls, n, (const fe_t *)ts, (const uint32_t *)d_row, d_cnt, cap - 1);
    if (S->field == 0) SRS_LAUNCH((k_m_emit<Fr>), (blocks, gy), (256), 0, st, (const fe_t *)ts, n, (const uint32_t *)d_row, (const uint32_t *)d_cnt, cap - 1, ms);
    else SRS_LAUNCH((k_m_emit<Fq>), (blocks, gy), (256), 0, st, (const fe_t *)ts, n, (const uint32_t *)d_row, (const uint32_t *)d_cnt, cap - 1, ms);
    return 0;
}

// Round 2, evaluate_coefficient_2 (lookup.rs:350-365): ONE launch reads l, t, m of every lookup from their places and writes h, g to theirs
void sps_lookup_round_2(Structure *S, fe_t *W_dev, const fe_t &r, hipStream_t st) {
    const size_t L = S->num_lookups, n = S->rows;
    if (!L) return;
    const fe_t *l = W_dev + S->num_advice * n, *t = l + L * n, *m = t + L * n;
    fe_t *h = W_dev + (S->num_advice + 3 * L) * n, *g = h + L * n;
    prof::Scope ps("lookup_hg", st, n * L);
    const uint32_t gx = (uint32_t)((n + HG_THREADS * HG_CHUNK - 1) / (HG_THREADS * HG_CHUNK));
    if (S->field == 0) SRS_LAUNCH((k_lookup_hg<Fr>), (gx, 2, (uint32_t)L), (HG_THREADS), 0, st, l, t, m, r, (uint32_t)n, h, g);
    else SRS_LAUNCH((k_lookup_hg<Fq>), (gx, 2, (uint32_t)L), (HG_THREADS), 0, st, l, t, m, r, (uint32_t)n, h, g);
}

// Arguments::evaluate_h_g (lookup.rs:305-317) for one lookup: h = 1/(l + r), g = m/(t + r)
void lookup_coeff_2(int field, const fe_t *l, const fe_t *t, const fe_t *m, const fe_t &r, size_t n, fe_t *h, fe_t *g, hipStream_t st) {
    if (!n) return;
    prof::Scope ps("lookup_hg", st, n);
    const uint32_t gx = (uint32_t)((n + HG_THREADS * HG_CHUNK - 1) / (HG_THREADS * HG_CHUNK));
    if (field == 0) SRS_LAUNCH((k_lookup_hg<Fr>), (gx, 2), (HG_THREADS), 0, st, l, t, m, r, (uint32_t)n, h, g);
    else SRS_LAUNCH((k_lookup_hg<Fq>), (gx, 2), (HG_THREADS), 0, st, l, t, m, r, (uint32_t)n, h, g);
}

void assigned_invert(int field, const fe_t *num, const fe_t *den, const uint8_t *has_den, size_t n, fe_t *out, hipStream_t st) {
    if (!n) return;
    const uint32_t gx = (uint32_t)((n + HG_THREADS * HG_CHUNK - 1) / (HG_THREADS * HG_CHUNK));
    if (field == 0) SRS_LAUNCH((k_assigned_invert<Fr>), (gx), (HG_THREADS), 0, st, num, den, has_den, (uint32_t)n, out);
    else SRS_LAUNCH((k_assigned_invert<Fq>), (gx), (HG_THREADS), 0, st, num, den, has_den, (uint32_t)n, out);
}

// PlonkStructure::is_sat_log_derivative (src/plonk/mod.rs:366-398) on the concatenated witness:
// number of lookups i whose sum_row (h_i - g_i) != 0; h_i / g_i are columns 2 i / 2 i + 1 of the LAST round.
size_t log_derivative_mismatches(Structure *S, const fe_t *W_dev, hipStream_t st) {
    const size_t L = S->num_lookups;
    if (!L) return 0;
    FieldOps f{S->field};
    const uint32_t n = (uint32_t)S->rows, blocks = std::min<uint32_t>((n + 255) / 256, 256);
    const fe_t *last = W_dev + (S->num_advice + 3 * L) * S->rows;
    fe_t *d_part = nullptr;
    SRS_HIP_CHECK(hipMalloc((void **)&d_part, L * blocks * sizeof(fe_t)));
    std::vector<fe_t> part(L * blocks);
    try {
        for (size_t i = 0; i < L; ++i) {
            const fe_t *h = last + (2 * i) * S->rows, *g = last + (2 * i + 1) * S->rows;
            if (S->field == 0) SRS_LAUNCH((k_sum_diff<Fr>), (blocks), (256), 0, st, h, g, n, d_part + i * blocks);
            else SRS_LAUNCH((k_sum_diff<Fq>), (blocks), (256), 0, st, h, g, n, d_part + i * blocks);
        }
        SRS_HIP_CHECK(hipMemcpyAsync(part.data(), d_part, part.size() * sizeof(fe_t), hipMemcpyDeviceToHost, st));
        SRS_HIP_CHECK(hipStreamSynchronize(st));
    } catch (...) { (void)hipFree(d_part); throw; }
    (void)hipFree(d_part);
    size_t bad = 0;
    for (size_t i = 0; i < L; ++i) {
        fe_t acc = f.zero();
        for (uint32_t b = 0; b < blocks; ++b) acc = f.add(acc, part[i * blocks + b]);
        if (!f.is_zero(acc)) ++bad;
    }
    return bad;
}

int lincomb(int field, fe_t *out, const fe_t *const *w_dev, const fe_t *coefs, size_t J, size_t n, hipStream_t st, std::string &err,
            uint32_t rank, uint32_t world) {
    if (J == 0 || J > JMAX) { err = "unsupported number of witnesses"; return 4; }
    if (world <= 1) { rank = 0; world = 1; }
    n = Stripes{rank, world}.count(n);         // the elements of this rank's stripes
    if (!n) return 0;
    LincombArgs a;
    a.J = (uint32_t)J;
    for (uint32_t j = 0; j < JMAX; ++j) {
        a.w[j] = j < J ? w_dev[j] : nullptr;
        a.coef[j] = j < J ? coefs[j] : Fr::zero();
    }
    uint32_t blocks = (uint32_t)std::min<size_t>((n + 255) / 256, 256 * 16);
    FieldOps f{field};
    fe_t sum = f.zero();
    for (size_t j = 0; j < J; ++j) sum = f.add(sum, coefs[j]);
    const bool affine = J >= 2 && f.is_zero(f.sub(sum, f.one()));
    if (field == 0) {
        if (affine) SRS_LAUNCH((k_lincomb<Fr, true>), (blocks), (256), 0, st, out, a, n, rank, world);
        else SRS_LAUNCH((k_lincomb<Fr, false>), (blocks), (256), 0, st, out, a, n, rank, world);
    } else {
        if (affine) SRS_LAUNCH((k_lincomb<Fq, true>), (blocks), (256), 0, st, out, a, n, rank, world);
        else SRS_LAUNCH((k_lincomb<Fq, false>), (blocks), (256), 0, st, out, a, n, rank, world);
    }
    return 0;
}

int lincomb_rows(int field, fe_t *out, const fe_t *const *w_dev, const fe_t *coefs, size_t J, const uint32_t *rows_dev, size_t n_rows, size_t cols,
                 size_t col_len, hipStream_t st, std::string &err) {
    if (J == 0 || J > JMAX) { err = "unsupported number of witnesses"; return 4; }
    if (!n_rows || !cols) return 0;
    LincombArgs a;
    a.J = (uint32_t)J;
    for (uint32_t j = 0; j < JMAX; ++j) {
        a.w[j] = j < J ? w_dev[j] : nullptr;
        a.coef[j] = j < J ? coefs[j] : Fr::zero();
    }
    const uint32_t blocks = (uint32_t)((n_rows * cols + 255) / 256);
    if (field == 0) SRS_LAUNCH((k_lincomb_rows<Fr>), (blocks), (256), 0, st, out, a, rows_dev, n_rows, cols, col_len);
    else SRS_LAUNCH((k_lincomb_rows<Fq>), (blocks), (256), 0, st, out, a, rows_dev, n_rows, cols, col_len);
    return 0;
}

}  // namespace rowprog
}  // namespace srs
