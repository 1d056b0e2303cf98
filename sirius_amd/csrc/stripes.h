// stripes.h -- the block-cyclic sharding of every multi-GPU path, stated once.
//
// A vector (key bases, scalars, the rows of a column) is cut into stripes of 2^STRIPE_LOG elements and stripe s belongs to rank
// s % world.  A rank keeps its stripes compactly: its t-th owned element has LOCAL index t.  Counts, the local -> global index map
// and the decomposition of a range into at most three strided runs (what the host turns into copies and memsets) all live here.
// Plain integer C++, host and device, no HIP types or calls: the kernels, the row programs compiled at run time (jit.hip embeds this
// file) and tests/emu/stripes_check.cpp (g++ with sanitizers, a 4-element stripe, every case) compile this very text.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC_RTC__)
#include <stddef.h>       // size_t: hiprtc declares it itself and has no such header
#endif

#if defined(__HIP__)
#define SRS_STRIPES_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SRS_STRIPES_HD inline __attribute__((always_inline))
#endif

namespace srs {

constexpr uint32_t STRIPE_LOG = 10;       // the only definition: key entries, scalars and rows are sharded alike

// `rows` pieces of `width` elements: piece r starts at global offset global + r * world * 2^LOG and at local offset local + r * 2^LOG
// (rows > 1 only for whole stripes, width = 2^LOG)
struct Run {
    size_t global, local, width, rows;
};

template <uint32_t LOG>
struct StripesT {
    uint32_t rank, world;                 // world <= 1: everything is mine
    static constexpr size_t S = (size_t)1 << LOG;

    SRS_STRIPES_HD bool owns(size_t i) const { return world <= 1 || (i >> LOG) % world == rank; }

    // global index of this rank's local element `local` (in the caller's index type: the row kernels stay on 32 bits)
    template <class T>
    SRS_STRIPES_HD T global_index(T local) const {
        if (world <= 1) return local;
        const T s = local >> LOG, o = local & ((1u << LOG) - 1);
        return ((s * world + rank) << LOG) + o;
    }

    // this rank's elements of [0, n) / of [a, b)
    SRS_STRIPES_HD size_t count(size_t n) const {
        if (world <= 1) return n;
        const size_t full = n >> LOG;
        return (full / world + (rank < full % world ? 1 : 0)) * S + (rank == full % world ? n & (S - 1) : 0);
    }
    SRS_STRIPES_HD size_t count(size_t a, size_t b) const { return count(b) - count(a); }

    // this rank's elements of [a, b) as at most three runs in ascending order: the partial first stripe, the whole stripes as one
    // strided block, the partial last stripe.  -> number of runs
    SRS_STRIPES_HD int runs(size_t a, size_t b, Run out[3]) const {
        if (a >= b) return 0;
        if (world <= 1) {
            out[0] = Run{a, a, b - a, 1};
            return 1;
        }
        int k = 0;
        size_t local = count(a), s = a >> LOG;
        const size_t last = b >> LOG;                      // [last * S, b) is the partial last stripe
        if (s == last) {                                   // inside one stripe
            if (s % world == rank) out[k++] = Run{a, local, b - a, 1};
            return k;
        }
        if (a & (S - 1)) {
            if (s % world == rank) {
                out[k++] = Run{a, local, (s + 1) * S - a, 1};
                local += (s + 1) * S - a;
            }
            ++s;
        }
        const size_t s0 = s + (rank + world - s % world) % world;      // my first whole stripe of [s, last)
        if (s0 < last) {
            const size_t rows = (last - s0 + world - 1) / world;
            out[k++] = Run{s0 * S, local, S, rows};
            local += rows * S;
        }
        if ((b & (S - 1)) && last % world == rank) out[k++] = Run{last * S, local, b - last * S, 1};
        return k;
    }

    // fn(global, local, width) for every contiguous piece of runs(a, b), ascending
    template <class Fn>
    SRS_STRIPES_HD void each_piece(size_t a, size_t b, Fn fn) const {
        Run run[3];
        const int n = runs(a, b, run);
        for (int i = 0; i < n; ++i)
            for (size_t r = 0; r < run[i].rows; ++r) fn(run[i].global + r * world * S, run[i].local + r * S, run[i].width);
    }
};

using Stripes = StripesT<STRIPE_LOG>;

}  // namespace srs
