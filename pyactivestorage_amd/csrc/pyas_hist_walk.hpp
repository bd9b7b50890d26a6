// pyas_hist_walk.hpp — what the counting kernels share: binned counts
// (pyas_hist.hip) and the digit counts of the radix select (pyas_select.hip).
// The accumulators below go through the runs and the per-element walk of
// pyas_stat_walk.hpp; which slot an element adds to is the business of their
// rule `B`.  hist_row and hist_flush: the table row of an output, and the LDS
// table's way into it.
#pragma once

#include <hip/hip_runtime.h>

#include "pyas_stat_walk.hpp"   // the tile share, the runs, the per-element walk

namespace pyas {

typedef unsigned long long hist_u64;

// The LDS-table kernels: at most 128 VGPRs (4 waves per SIMD; 1-byte types unpack 16 values per load and get
// 256), and every call inlined: their six run variants put them beyond the inliner's budget, and one call left
// standing sends the argument block to scratch
#define PYAS_HIST_WAVES(T) __attribute__((amdgpu_waves_per_eu(sizeof(T) > 1 ? 4 : 2, 8), flatten))

// The accumulators.  `B` is the rule that turns values into slots of a table
// row: b.slots<N>(x, ok, idx) gives the slots of N values (ok[k]: x[k] is
// selected and unmasked; the other slots lie inside the row but mean nothing),
// b.n the row's counting slots (three more follow: below, above, nan).

// Counts into this lane's copy of the LDS table.  A masked element adds to a
// spare slot after the row's (never flushed), so the add needs no branch.
template <typename B>
struct CountLds {
    B b;
    uint8_t *tab;          // this lane's copy of slot 0
    int sh;                // log2(copies) + 2: byte shift of a slot
    template <int N, typename T>
    __device__ __forceinline__ void add(const T *x, const bool *ok) const {
        int idx[N];
        b.template slots<N>(x, ok, idx);
        const int spare = b.n + 3;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const uint32_t s = (uint32_t)(ok[k] ? idx[k] : spare);
            __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(tab + (s << sh)), 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    // N values under mask mode M (0 none, kMaskRange, kMaskAll)
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const MaskT<T> &mk) const {
        bool ok[N];
#pragma unroll
        for (int k = 0; k < N; ++k) ok[k] = M ? !mk.template masked_m<M>(x[k]) : true;
        add<N>(x, ok);
    }
};

// one global atomic per element (a lane per output)
template <typename B>
struct CountLane {
    B b;
    hist_u64 *row;
    template <int N, typename T>
    __device__ __forceinline__ void add(const T *x, const bool *ok) const {
        int idx[N];
        b.template slots<N>(x, ok, idx);
#pragma unroll
        for (int k = 0; k < N; ++k)
            if (ok[k]) __hip_atomic_fetch_add(row + idx[k], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// every active lane of the wave adds to the same row: equal slots add once
template <typename B>
struct CountWave {
    B b;
    hist_u64 *row;
    template <int N, typename T>
    __device__ __forceinline__ void add(const T *x, const bool *ok) const {
        int idx[N];
        b.template slots<N>(x, ok, idx);
        const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            uint64_t rem = __ballot(ok[k]);
            while (rem) {
                const int leader = __builtin_ctzll(rem);
                const int sl = __shfl(idx[k], leader);
                const uint64_t m = __ballot(ok[k] && idx[k] == sl);
                if (lane == leader)
                    __hip_atomic_fetch_add(row + sl, (hist_u64)__builtin_popcountll(m), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT);
                rem &= ~m;
            }
        }
    }
};

// the table row of output o (C order over the kept selected dims) of chunk c
__device__ __forceinline__ int64_t hist_row(const int64_t *out_offsets, const int64_t *out_index, int64_t c, int64_t o) {
    if (!out_offsets) return 0;   // every dim reduced, one output
    const int64_t k = out_offsets[c] + o;
    return out_index ? out_index[k] : k;
}

// Sum the copies of every slot into the global row and leave the LDS table
// zero.  Every thread of the workgroup calls it.
__device__ __forceinline__ void hist_flush(uint32_t *tab, int slots, int shift, hist_u64 *row) {
    __syncthreads();
    const int copies = 1 << shift;
    for (int s = threadIdx.x; s < slots; s += kBlock) {
        hist_u64 sum = 0;
        for (int k = 0; k < copies; ++k) {
            uint32_t *p = tab + (s << shift) + ((k + threadIdx.x) & (copies - 1));   // lanes on different banks
            sum += *p;
            *p = 0;
        }
        if (sum) __hip_atomic_fetch_add(row + s, sum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
}

}  // namespace pyas
