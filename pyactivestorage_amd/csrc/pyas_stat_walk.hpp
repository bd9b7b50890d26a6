// pyas_stat_walk.hpp — the scaffolding the statistics kernels share
// (pyas_moments, pyas_weighted, pyas_comoments, pyas_trend, pyas_hist,
// pyas_select): a tile's share of a selection, the contiguous runs, the
// per-element walk of the counting kernels, the LDS offset map, and how lane
// records become a workgroup's record.  A statistic file keeps what is its
// own: the accumulator, the record's merge, its side tables and its kernels.
//
// An accumulator `Acc` takes elements two ways: the runs call
// acc.add_n<N, M>(x, mk) (N values under mask mode M: 0 none, kMaskRange,
// kMaskAll), stat_walk calls acc.add<N>(x, ok) (ok[k]: x[k] is selected and
// unmasked).  A record `R` comes with a merge trait `M`: M::merged(a, b) (a
// then b: the order matters to the last bit) and M::shfl_xor(p, m) (the
// record of the lane at distance m).
//
// What is deliberately not here ("One walk skeleton"): the
// "one contiguous run?" loop of the `*_full` kernels, the output loops of the
// record `*_axes` kernels and the walks of pyas_moments.hip.  Moved into a
// function they compile to other registers, so each kernel keeps its copy.
#pragma once

#include <hip/hip_runtime.h>

#include "pyas_kernels.hpp"   // ldg16, unpack16, unshuffle16, RadixCounter, decompose, all_masked

namespace pyas {

// ---------------------------------------------------------------------------
// a workgroup's share
// ---------------------------------------------------------------------------
// the mask mode of a run: which rules its elements are checked against
__device__ __forceinline__ int mask_mode(bool masked, uint32_t flags) {
    return !masked || flags == 0 ? 0 : (flags & (PYAS_MASK_EQ0 | PYAS_MASK_EQ1)) ? kMaskAll : kMaskRange;
}

// tile t of bpc: elements [e0, e1) of the selection, whole 16-element groups
__device__ __forceinline__ void tile_share(int64_t total, int64_t bpc, int64_t t, int64_t &e0, int64_t &e1) {
    const int64_t per = (((total + bpc - 1) / bpc) + 15) & ~(int64_t)15;
    e0 = t * per < total ? t * per : total;
    e1 = e0 + per < total ? e0 + per : total;
}

// the selected extents of the kept and of the reduced (`red`) dims
__device__ __forceinline__ void axes_extents(const Sel &s, int ndim, uint32_t red, int64_t &n_keep, int64_t &n_red) {
    n_keep = 1;
    n_red = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
        if (d < ndim) {
            if ((red >> d) & 1u) n_red *= s.cnt[d];
            else n_keep *= s.cnt[d];
        }
    }
}

// one element, its byte order a run-time flag
template <typename T, bool SHUF>
__device__ __forceinline__ T load_elem_bsw(const uint8_t *base, int64_t n, int64_t i, bool bsw) {
    return bsw ? load_elem<T, SHUF, true>(base, n, i) : load_elem<T, SHUF, false>(base, n, i);
}

// ---------------------------------------------------------------------------
// contiguous runs (the layout of run_plain / run_shuffled in pyas_kernels.hpp)
// ---------------------------------------------------------------------------
// Chunk elements [m0, m1): 16-B loads, register double-buffered, with scalar
// head and tail.  A lane's vectors come in increasing order.
template <typename T, bool BSWAP, int M, typename Acc>
__device__ __forceinline__ void stat_run_plain(const uint8_t *base, int64_t m0, int64_t m1, Acc &acc,
                                               const MaskT<T> &mk) {
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
            // the next step's loads are in flight while this step is consumed
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
__device__ __forceinline__ void stat_run_shuffled(const uint8_t *base, int64_t n, int64_t i0, int64_t i1, Acc &acc,
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
__device__ __forceinline__ void stat_run(int mode, const uint8_t *base, int64_t n, int64_t i0, int64_t i1, Acc &acc,
                                         const MaskT<T> &mk) {
    if constexpr (SHUF && sizeof(T) > 1) {
        if (mode == 0) stat_run_shuffled<T, BSWAP, 0>(base, n, i0, i1, acc, mk);
        else if (mode == kMaskRange) stat_run_shuffled<T, BSWAP, kMaskRange>(base, n, i0, i1, acc, mk);
        else stat_run_shuffled<T, BSWAP, kMaskAll>(base, n, i0, i1, acc, mk);
    } else {
        if (mode == 0) stat_run_plain<T, BSWAP, 0>(base, i0, i1, acc, mk);
        else if (mode == kMaskRange) stat_run_plain<T, BSWAP, kMaskRange>(base, i0, i1, acc, mk);
        else stat_run_plain<T, BSWAP, kMaskAll>(base, i0, i1, acc, mk);
    }
}

// ---------------------------------------------------------------------------
// per-element walks
// ---------------------------------------------------------------------------
// Positions q0, q0 + stride, ... < n_pos over the dims in `dmask` (rc: the
// radix counter at q0; base_o: the other dims' part), 4 loads in flight.
template <typename T, bool SHUF, typename Acc>
__device__ __forceinline__ void stat_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t dmask,
                                          const Decomp &base_o, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                          int64_t stride, bool bsw, const MaskT<T> &mk, Acc &acc) {
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
        for (int u = 0; u < U; ++u) x[u] = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od[u].mem, bsw);
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ok[u] = !all_masked(mk, r.tab, od[u], x[u]);
        acc.template add<U>(x, ok);
    }
    for (; q < n_pos; q += stride) {
        Decomp od = base_o;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od);
        rc.advance();
        const T x = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od.mem, bsw);
        const bool ok = !all_masked(mk, r.tab, od, x);
        acc.template add<1>(&x, &ok);
    }
}

// The reduced positions' element offsets in LDS (no vector mask tables), once
// per workgroup: every thread calls this.  roff holds n_red entries (each
// kernel sizes its own map: kMomRoff, kComRoff).
__device__ __forceinline__ void stage_roff(const ReduceArgs &r, const Sel &s, uint32_t red, int64_t n_red,
                                           int32_t *roff) {
    for (int64_t q = threadIdx.x; q < n_red; q += kBlock) {
        Decomp o{0, {0, 0}};
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, red, q, o);
        roff[q] = (int32_t)o.mem;   // |offset| < chunk elements < 2^31
    }
    __syncthreads();
}

// ---------------------------------------------------------------------------
// records: lanes -> wave -> workgroup -> out
// ---------------------------------------------------------------------------
// Every lane of the wave participates; every lane ends with the wave's record
// (pairs at distance 1, 2, 4, ...: the lower lane's side first).
template <typename R, typename M>
__device__ __forceinline__ void rec_wave_merge(R &p) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        const R q = M::shfl_xor(p, m);
        p = (lane & m) ? M::merged(q, p) : M::merged(p, q);
    }
}

// Wave merge, then the 4 waves in wave order; valid in thread 0.
template <typename R, typename M>
__device__ __forceinline__ void rec_block_merge(R &p) {
    __shared__ R s_w[kBlock / kWave];
    rec_wave_merge<R, M>(p);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kBlock / kWave; ++k) p = M::merged(p, s_w[k]);
    }
}

// The end of a `*_full` kernel (workgroup = tile blockIdx.x % bpc of chunk c):
// the workgroup's record to its tile slot, or to the chunk's output when the
// chunk is one tile.  A: the kernel's arguments (bpc, tiles, out, out_offsets).
template <typename M, typename Acc, typename A>
__device__ __forceinline__ void rec_store_full(const Acc &acc, const A &a, int64_t c) {
    auto p = acc.finish();
    rec_block_merge<decltype(p), M>(p);
    if (threadIdx.x == 0) {
        if (a.bpc > 1) a.tiles[blockIdx.x] = p;
        else a.out[a.out_offsets ? a.out_offsets[c] : c] = p;
    }
}

}  // namespace pyas
