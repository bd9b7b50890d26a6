// pyas_moments.hip — second-moment kernels behind Active.var / Active.std
// (pyas_moments_axes and the two moments combines of include/pyas.h).
//
// One pass over the same bytes a mean reads.  Per lane: a shift K (the first
// unmasked value the lane meets, as f64), n, s1 = sum (x-K), s2 = sum (x-K)^2
// in f64 with FMA; a lane finishes to (n, K + s1/n, s2 - s1^2/n).  Everything
// above a lane (lanes of a wave, waves, tiles, chunks, chunk layers) merges
// pyas_moments records with Chan's formula in a fixed order, so a result is
// bit-identical from run to run and does not depend on the launch geometry.
// Masked elements are excluded by select (never multiplied by 0).
//
// k_moments_full : every dim reduced, one workgroup per (chunk, tile).  A whole
//                  chunk or a selection that is one contiguous run streams
//                  16-B loads, register double-buffered, with scalar head and
//                  tail; anything else walks per element.
// k_moments_axes : partial axes, one record per kept output.  Innermost dim
//                  kept: a lane per output (adjacent lanes read adjacent
//                  elements); innermost dim reduced: a wave per output.
// Both are templated on the dtype and shuffled-or-not only; byte order, mask
// rules and selection kind are run-time branches (18 kernels each).
#include <hip/hip_runtime.h>

#include "pyas_kernels.hpp"   // ldg16, unpack16, unshuffle16, RadixCounter, decompose, all_masked
#include "pyas_records.hpp"   // the tile / segment / grid combines

namespace pyas {

struct MomMerge {
    // a then b (the order matters to the last bit, so every caller fixes it)
    static __device__ __forceinline__ pyas_moments merged(const pyas_moments &a, const pyas_moments &b) {
        const double na = (double)a.count, nb = (double)b.count;
        const double d = b.mean - a.mean;
        const double w = nb / (na + nb);
        pyas_moments r;
        r.count = a.count + b.count;
        r.mean = a.mean + d * w;
        r.m2 = a.m2 + b.m2 + d * d * na * w;
        r.reserved = 0;
        if (b.count == 0) r = a;         // an empty side is skipped, not multiplied through
        else if (a.count == 0) r = b;
        return r;
    }
};

struct MomAcc {
    double K, s1, s2;
    uint32_t n;
    __device__ __forceinline__ void init() { K = 0.0; s1 = 0.0; s2 = 0.0; n = 0; }
    // one element; ok = selected and unmasked
    __device__ __forceinline__ void add_one(double x, bool ok) {
        K = (ok && n == 0) ? x : K;
        const double d = ok ? x - K : 0.0;
        s1 += d;
        s2 = __builtin_fma(d, d, s2);
        n += ok ? 1u : 0u;
    }
    // K is set (n > 0)
    __device__ __forceinline__ void add_next(double x, bool ok) {
        const double d = ok ? x - K : 0.0;
        s1 += d;
        s2 = __builtin_fma(d, d, s2);
        n += ok ? 1u : 0u;
    }
    // N values; M: mask mode (0 none, kMaskRange, kMaskAll).  Once every lane
    // that runs this call has its K, the shift is no longer looked for.
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const MaskT<T> &mk) {
        if (__builtin_expect(__ballot(n == 0) != 0, 0)) {
#pragma unroll
            for (int k = 0; k < N; ++k) add_one((double)x[k], M ? !mk.template masked_m<M>(x[k]) : true);
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) add_next((double)x[k], M ? !mk.template masked_m<M>(x[k]) : true);
        }
    }
    __device__ __forceinline__ pyas_moments finish() const {
        pyas_moments p;
        p.reserved = 0;
        if (n == 0) {
            p.count = 0; p.mean = 0.0; p.m2 = 0.0;
        } else {
            const double mu = s1 / (double)n;
            const double m2 = __builtin_fma(-s1, mu, s2);
            p.count = (int64_t)n;
            p.mean = K + mu;
            p.m2 = m2 < 0.0 ? 0.0 : m2;   // a rounding residue; NaN stays NaN
        }
        return p;
    }
};

// Every lane of the wave participates; every lane ends with the wave's record
// (pairs at distance 1, 2, 4, ...: the lower lane's side first).
__device__ __forceinline__ void mom_wave_merge(pyas_moments &p) {
    const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
    for (int m = 1; m < kWave; m <<= 1) {
        pyas_moments q;
        q.count = shfl_xor(p.count, m);
        q.mean = shfl_xor(p.mean, m);
        q.m2 = shfl_xor(p.m2, m);
        q.reserved = 0;
        p = (lane & m) ? MomMerge::merged(q, p) : MomMerge::merged(p, q);
    }
}

// Wave merge, then the 4 waves in wave order; valid in thread 0.
__device__ __forceinline__ void mom_block_merge(pyas_moments &p) {
    __shared__ pyas_moments s_w[kBlock / kWave];
    mom_wave_merge(p);
    if ((threadIdx.x & (kWave - 1)) == 0) s_w[threadIdx.x / kWave] = p;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kBlock / kWave; ++k) p = MomMerge::merged(p, s_w[k]);
    }
}

// ---------------------------------------------------------------------------
// contiguous runs (the layout of run_plain / run_shuffled in pyas_kernels.hpp)
// ---------------------------------------------------------------------------
template <typename T, bool BSWAP, int M>
__device__ void mom_run_plain(const uint8_t *base, int64_t m0, int64_t m1, MomAcc &acc, const MaskT<T> &mk) {
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
            // the next step's loads are in flight while this step is reduced
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
template <typename T, bool BSWAP, int M>
__device__ void mom_run_shuffled(const uint8_t *base, int64_t n, int64_t i0, int64_t i1, MomAcc &acc,
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

template <typename T, bool SHUF, bool BSWAP>
__device__ __forceinline__ void mom_run(int mode, const uint8_t *base, int64_t n, int64_t i0, int64_t i1,
                                        MomAcc &acc, const MaskT<T> &mk) {
    if constexpr (SHUF && sizeof(T) > 1) {
        if (mode == 0) mom_run_shuffled<T, BSWAP, 0>(base, n, i0, i1, acc, mk);
        else if (mode == kMaskRange) mom_run_shuffled<T, BSWAP, kMaskRange>(base, n, i0, i1, acc, mk);
        else mom_run_shuffled<T, BSWAP, kMaskAll>(base, n, i0, i1, acc, mk);
    } else {
        if (mode == 0) mom_run_plain<T, BSWAP, 0>(base, i0, i1, acc, mk);
        else if (mode == kMaskRange) mom_run_plain<T, BSWAP, kMaskRange>(base, i0, i1, acc, mk);
        else mom_run_plain<T, BSWAP, kMaskAll>(base, i0, i1, acc, mk);
    }
}

template <typename T, bool SHUF>
__device__ __forceinline__ T mom_load(const uint8_t *base, int64_t n, int64_t i, bool bsw) {
    return bsw ? load_elem<T, SHUF, true>(base, n, i) : load_elem<T, SHUF, false>(base, n, i);
}

// Per-element walk of positions q0, q0 + stride, ... < n_pos over the dims in
// `dmask` (rc: the radix counter at q0), 4 loads in flight.
template <typename T, bool SHUF>
__device__ __forceinline__ void mom_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t dmask,
                                         const Decomp &base_o, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                         int64_t stride, bool bsw, const MaskT<T> &mk, MomAcc &acc) {
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
        for (int u = 0; u < U; ++u) x[u] = mom_load<T, SHUF>(base, r.chunk_elems, od[u].mem, bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one((double)x[u], !all_masked(mk, r.tab, od[u], x[u]));
    }
    for (; q < n_pos; q += stride) {
        Decomp od = base_o;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od);
        rc.advance();
        const T x = mom_load<T, SHUF>(base, r.chunk_elems, od.mem, bsw);
        acc.add_one((double)x, !all_masked(mk, r.tab, od, x));
    }
}

// The same walk with the reduced positions' element offsets already in LDS (no
// vector mask tables): per element one LDS read, one add, one load.
constexpr int kMomRoff = 4096;   // reduced positions kept in LDS (int32, 16 KiB)
template <typename T, bool SHUF>
__device__ __forceinline__ void mom_walk_lds(const uint8_t *base, int64_t chunk_elems, const int32_t *roff,
                                             int64_t base_mem, int64_t q0, int64_t n_pos, int64_t stride, bool bsw,
                                             const MaskT<T> &mk, MomAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = mom_load<T, SHUF>(base, chunk_elems, base_mem + roff[q + u * stride], bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one((double)x[u], !mk.masked(x[u]));
    }
    for (; q < n_pos; q += stride) {
        const T x = mom_load<T, SHUF>(base, chunk_elems, base_mem + roff[q], bsw);
        acc.add_one((double)x, !mk.masked(x));
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_moments_full(MomentsArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, t = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const bool tabs = r.tab.on[0] || r.tab.on[1];
    // One contiguous run?  From the innermost dim: whole dims, then one
    // unit-step range, then single indices.
    int64_t total = 1, m0 = 0;
    bool contig = !tabs, inner_full = true;
#pragma unroll
    for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
        if (d < r.ndim) {
            const int64_t cnt = s.cnt[d];
            total *= cnt;
            if (s.step[d] == 0) contig = false;
            if (cnt != 1 && (!inner_full || s.step[d] != 1)) contig = false;
            m0 += (int64_t)s.start[d] * r.cstride[d];
            if (!(s.start[d] == 0 && s.step[d] == 1 && cnt == r.shape[d])) inner_full = false;
        }
    }
    // this tile's share of the selection: whole 16-element groups
    const int64_t per = (((total + a.bpc - 1) / a.bpc) + 15) & ~(int64_t)15;
    const int64_t e0 = t * per < total ? t * per : total;
    const int64_t e1 = e0 + per < total ? e0 + per : total;
    MomAcc acc;
    acc.init();
    if (e0 < e1) {
        if (contig) {
            const uint32_t f = r.mask.flags;
            const int mode = !a.masked || f == 0 ? 0 : (f & (PYAS_MASK_EQ0 | PYAS_MASK_EQ1)) ? kMaskAll : kMaskRange;
            if (a.bswap) mom_run<T, SHUF, true>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
            else mom_run<T, SHUF, false>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
        } else if (e0 + threadIdx.x < e1) {
            const uint32_t all = (1u << r.ndim) - 1u;
            RadixCounter rc;
            rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
            const Decomp zero{0, {0, 0}};
            mom_walk<T, SHUF>(r, base, s, all, zero, rc, e0 + threadIdx.x, e1, kBlock, a.bswap, mk, acc);
        }
    }
    pyas_moments p = acc.finish();
    mom_block_merge(p);
    if (threadIdx.x == 0) {
        if (a.bpc > 1) a.tiles[blockIdx.x] = p;
        else a.out[a.out_offsets ? a.out_offsets[c] : c] = p;
    }
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_moments_axes(MomentsArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep = 1, n_red = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
        if (d < r.ndim) {
            if ((red >> d) & 1u) n_red *= s.cnt[d];
            else n_keep *= s.cnt[d];
        }
    }
    pyas_moments *out = a.out + a.out_offsets[c];
    // the reduced positions' offsets, once per workgroup, when they fit
    __shared__ int32_t s_roff[kMomRoff];
    const bool mapped = !(r.tab.on[0] || r.tab.on[1]) && n_red <= kMomRoff;   // uniform
    if (mapped) {
        for (int64_t q = threadIdx.x; q < n_red; q += kBlock) {
            Decomp o{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, red, q, o);
            s_roff[q] = (int32_t)o.mem;   // |offset| < chunk elements < 2^31
        }
        __syncthreads();
    }
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            MomAcc acc;
            acc.init();
            if (n_red > 0) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    mom_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, 0, n_red, 1, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, 0, 1);
                    mom_walk<T, SHUF>(r, base, s, red, bo, rc, 0, n_red, 1, a.bswap, mk, acc);
                }
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            MomAcc acc;
            acc.init();
            if (lane < n_red) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    mom_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, lane, n_red, kWave, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                    mom_walk<T, SHUF>(r, base, s, red, bo, rc, lane, n_red, kWave, a.bswap, mk, acc);
                }
            }
            pyas_moments p = acc.finish();
            mom_wave_merge(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_moments_full(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_moments_full), a, shuf, grid, 0, st)
}

hipError_t launch_moments_axes(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_moments_axes), a, shuf, grid, 0, st)
}

// the combines: pyas_records.hpp over the record and MomMerge
hipError_t launch_moments_tiles(const pyas_moments *tiles, int64_t tpc, int64_t n_chunks,
                                const int64_t *out_offsets, pyas_moments *out, hipStream_t st) {
    return launch_rec_tiles<pyas_moments, MomMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

hipError_t launch_moments_segments(const pyas_moments *in, const int64_t *index, const int64_t *seg,
                                   int64_t n_seg, pyas_moments *out, hipStream_t st) {
    return launch_rec_segments<pyas_moments, MomMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_moments_grid(const pyas_moments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                               pyas_moments *out, hipStream_t st) {
    return launch_rec_grid<pyas_moments, MomMerge>(in, g, n_out, n_layers, out, st);
}

}  // namespace pyas
