// pyas_hist_walk.hpp — the walkers shared by the counting kernels: binned
// counts (pyas_hist.hip) and the digit counts of the radix select
// (pyas_select.hip).  What an element adds to is the accumulator's business
// (`Acc`): the runs call acc.add_n<N, M>(x, mk) (N values under mask mode M),
// the per-element walk acc.add<N>(x, ok).
#pragma once

#include <hip/hip_runtime.h>

#include "pyas_kernels.hpp"   // ldg16, unpack16, unshuffle16, RadixCounter, decompose, all_masked

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

// ---------------------------------------------------------------------------
// contiguous runs (the layout of mom_run_plain / mom_run_shuffled)
// ---------------------------------------------------------------------------
template <typename T, bool BSWAP, int M, typename Acc>
__device__ __forceinline__ void hist_run_plain(const uint8_t *base, int64_t m0, int64_t m1, const Acc &acc, const MaskT<T> &mk) {
    constexpr int ES = sizeof(T);
    constexpr int N = 16 / ES;
    const int tid = threadIdx.x;
    const int64_t b0 = m0 * ES, b1 = m1 * ES;               // byte range in the chunk
    const int64_t mis = (int64_t)((uintptr_t)base & 15);
    const int64_t a0 = ((b0 + mis + 15) & ~(int64_t)15) - mis;  // first 16-B aligned byte
    const int64_t a1 = ((b1 + mis) & ~(int64_t)15) - mis;
    if (a0 >= a1) {
        for (int64_t i = m0 + tid; i < m1; i += kBlock) {
            const T v = load_plain<T, BSWAP>(base, i);
            acc.template add_n<1, M>(&v, mk);
        }
        return;
    }
    const int64_t nhead = (a0 - b0) / ES, ntail = (b1 - a1) / ES;
    if (tid < nhead) {
        const T v = load_plain<T, BSWAP>(base, m0 + tid);
        acc.template add_n<1, M>(&v, mk);
    }
    if (tid < ntail) {
        const T v = load_plain<T, BSWAP>(base, m1 - ntail + tid);
        acc.template add_n<1, M>(&v, mk);
    }
    const uint4 *v = reinterpret_cast<const uint4 *>(base + a0);
    const int64_t nvec = (a1 - a0) / 16;
    constexpr int U = 4;
    constexpr int64_t STEP = (int64_t)U * kBlock;
    const int64_t nsteps = nvec / STEP;
    auto consume = [&](const uint4 *r) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            T x[N];
            unpack16<T, BSWAP>(r[u], x);
            acc.template add_n<N, M>(x, mk);
        }
    };
    if (nsteps > 0) {
        uint4 cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = ldg16(v + tid + u * kBlock);
        for (int64_t s = 0; s + 1 < nsteps; ++s) {
            // the next step's loads are in flight while this step is binned
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = ldg16(v + (s + 1) * STEP + tid + u * kBlock);
            consume(cur);
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
        consume(cur);
    }
    for (int64_t k = nsteps * STEP + tid; k < nvec; k += kBlock) {
        T x[N];
        unpack16<T, BSWAP>(ldg16(v + k), x);
        acc.template add_n<N, M>(x, mk);
    }
}

// Shuffled layout, chunk elements [i0, i1); n = elements in the chunk.
template <typename T, bool BSWAP, int M, typename Acc>
__device__ __forceinline__ void hist_run_shuffled(const uint8_t *base, int64_t n, int64_t i0, int64_t i1, const Acc &acc,
                                  const MaskT<T> &mk) {
    constexpr int ES = sizeof(T);
    const int tid = threadIdx.x;
    const bool vec_ok = (((uintptr_t)base & 15) == 0) && ((n & 15) == 0);
    const int64_t g0 = (i0 + 15) & ~(int64_t)15, g1 = i1 & ~(int64_t)15;
    if (!vec_ok || g0 >= g1) {
        for (int64_t i = i0 + tid; i < i1; i += kBlock) {
            const T v = load_shuffled<T, BSWAP>(base, n, i);
            acc.template add_n<1, M>(&v, mk);
        }
        return;
    }
    if (tid < g0 - i0) {
        const T v = load_shuffled<T, BSWAP>(base, n, i0 + tid);
        acc.template add_n<1, M>(&v, mk);
    }
    if (tid < i1 - g1) {
        const T v = load_shuffled<T, BSWAP>(base, n, g1 + tid);
        acc.template add_n<1, M>(&v, mk);
    }
    const int64_t ng = (g1 - g0) / 16;
    for (int64_t g = tid; g < ng; g += kBlock) {
        const int64_t i = g0 + g * 16;
        uint4 pl[ES];
#pragma unroll
        for (int b = 0; b < ES; ++b) pl[b] = ldg16(reinterpret_cast<const uint4 *>(base + (int64_t)b * n + i));
        T x[16];
        unshuffle16<T, BSWAP>(pl, x);
        acc.template add_n<16, M>(x, mk);
    }
}

template <typename T, bool SHUF, bool BSWAP, typename Acc>
__device__ __forceinline__ void hist_run(int mode, const uint8_t *base, int64_t n, int64_t i0, int64_t i1,
                                         const Acc &acc, const MaskT<T> &mk) {
    if constexpr (SHUF && sizeof(T) > 1) {
        if (mode == 0) hist_run_shuffled<T, BSWAP, 0>(base, n, i0, i1, acc, mk);
        else if (mode == kMaskRange) hist_run_shuffled<T, BSWAP, kMaskRange>(base, n, i0, i1, acc, mk);
        else hist_run_shuffled<T, BSWAP, kMaskAll>(base, n, i0, i1, acc, mk);
    } else {
        if (mode == 0) hist_run_plain<T, BSWAP, 0>(base, i0, i1, acc, mk);
        else if (mode == kMaskRange) hist_run_plain<T, BSWAP, kMaskRange>(base, i0, i1, acc, mk);
        else hist_run_plain<T, BSWAP, kMaskAll>(base, i0, i1, acc, mk);
    }
}

template <typename T, bool SHUF>
__device__ __forceinline__ T hist_load(const uint8_t *base, int64_t n, int64_t i, bool bsw) {
    return bsw ? load_elem<T, SHUF, true>(base, n, i) : load_elem<T, SHUF, false>(base, n, i);
}

// Per-element walk of positions q0, q0 + stride, ... < n_pos over the dims in
// `dmask` (rc: the radix counter at q0), 4 loads in flight.
template <typename T, bool SHUF, typename Acc>
__device__ __forceinline__ void hist_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t dmask,
                                          const Decomp &base_o, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                          int64_t stride, bool bsw, const MaskT<T> &mk, const Acc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp od[U];
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            od[u] = base_o;
            rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od[u]);
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = hist_load<T, SHUF>(base, r.chunk_elems, od[u].mem, bsw);
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ok[u] = !all_masked(mk, r.tab, od[u], x[u]);
        acc.template add<U>(x, ok);
    }
    for (; q < n_pos; q += stride) {
        Decomp od = base_o;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od);
        rc.advance();
        const T x = hist_load<T, SHUF>(base, r.chunk_elems, od.mem, bsw);
        const bool ok = !all_masked(mk, r.tab, od, x);
        acc.template add<1>(&x, &ok);
    }
}

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
