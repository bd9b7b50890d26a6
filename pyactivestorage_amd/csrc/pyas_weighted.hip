// pyas_weighted.hip — weighted-sum kernels behind Active.mean / Active.sum
// with weights= (pyas_wsum_axes and the two wsum combines of include/pyas.h).
//
// One pass over the same bytes a mean reads.  The weight of an element is the
// product of one factor per chunk dim, ((1 * f_0) * f_1) * ... in ascending dim
// order, f_d = pool[origin[c][d] + i_d] with i_d the element's index inside the
// chunk.  Per lane: n, sw = sum w, swx = sum w x in f64 (fma).  Everything above
// a lane (lanes of a wave, waves, tiles, chunks, chunk layers) adds records
// field by field in the fixed order of the moments records, so a result is
// bit-identical from run to run.  Masked elements are excluded by select
// (weight and value both; never multiplied by 0).
//
// k_wsum_full : every dim reduced, one workgroup per (chunk, tile).  A whole
//               chunk or a selection that is one contiguous run streams 16-B
//               loads, register double-buffered, with scalar head and tail.
//               Each lane carries the position of its next vector as one digit
//               per dim (a carry-propagating add per vector, no division); a
//               vector inside one innermost row takes the product of its outer
//               dims' factors once, a vector that straddles into the next row
//               takes that row's product too and selects per element.  Chunks
//               of rank <= 3 whose factors fit kWLds doubles read them from LDS
//               (staged once per workgroup), any other chunk from the pool in
//               global memory.  Anything that is not one run, and chunks whose
//               innermost extent is shorter than a vector, walk per element.
// k_wsum_axes : partial axes, one record per kept output, the per-element walk
//               with the factor look-ups added.  Innermost dim kept: a lane per
//               output; innermost dim reduced: a wave per output.
// Both are templated on the dtype and shuffled-or-not only (18 kernels each).
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // the tile / segment / grid combines
#include "pyas_stat_walk.hpp"   // the tile share, the record merges, load_elem_bsw
#include "pyas_wvec.hpp"        // WVec, VecPos, vec_weights, elem_weight, ws_mask_init, ws_keep

namespace pyas {

struct WsumMerge {
    static __device__ __forceinline__ pyas_wsum merged(const pyas_wsum &a, const pyas_wsum &b) {
        pyas_wsum r;
        r.count = a.count + b.count;
        r.sw = a.sw + b.sw;
        r.swx = a.swx + b.swx;
        r.reserved = 0;
        return r;
    }
    static __device__ __forceinline__ pyas_wsum shfl_xor(const pyas_wsum &p, int m) {
        pyas_wsum q;
        q.count = pyas::shfl_xor(p.count, m);
        q.sw = pyas::shfl_xor(p.sw, m);
        q.swx = pyas::shfl_xor(p.swx, m);
        q.reserved = 0;
        return q;
    }
};

struct WsAcc {
    double sw, swx;
    uint32_t n;
    __device__ __forceinline__ void init() { sw = 0.0; swx = 0.0; n = 0; }
    // one element of weight w; ok = selected and unmasked
    template <typename T>
    __device__ __forceinline__ void add(T x, double w, bool ok) {
        const T xs = ok ? x : (T)0;
        const double wv = ok ? w : 0.0;
        sw += wv;
        swx = __builtin_fma(wv, (double)xs, swx);
        n += ok ? 1u : 0u;
    }
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const double *w, const MaskT<T> &mk) {
#pragma unroll
        for (int k = 0; k < N; ++k) add(x[k], w[k], M ? !mk.template masked_m<M>(x[k]) : true);
    }
    __device__ __forceinline__ pyas_wsum finish() const {
        pyas_wsum p;
        p.count = (int64_t)n;
        p.sw = sw;
        p.swx = swx;
        p.reserved = 0;
        return p;
    }
};

// ---------------------------------------------------------------------------
// contiguous runs: factors by digit (pyas_wvec.hpp)
// ---------------------------------------------------------------------------
template <typename T, bool BSWAP, int M, bool WL, int K>
__device__ __forceinline__ void ws_run_plain(const uint8_t *base, int64_t m0, int64_t m1, WsAcc &acc, const MaskT<T> &mk,
                             const WVec<WL, K> &wv) {
    constexpr int ES = sizeof(T);
    constexpr int N = 16 / ES;
    const int tid = threadIdx.x;
    const int64_t b0 = m0 * ES, b1 = m1 * ES;               // byte range in the chunk
    const int64_t mis = (int64_t)((uintptr_t)base & 15);
    const int64_t a0 = ((b0 + mis + 15) & ~(int64_t)15) - mis;  // first 16-B aligned byte
    const int64_t a1 = ((b1 + mis) & ~(int64_t)15) - mis;
    auto one = [&](int64_t i) {
        const T x = load_plain<T, BSWAP>(base, i);
        const double w = elem_weight(wv, i);
        acc.template add_n<1, M>(&x, &w, mk);
    };
    if (a0 >= a1) {
        for (int64_t i = m0 + tid; i < m1; i += kBlock) one(i);
        return;
    }
    const int64_t nhead = (a0 - b0) / ES, ntail = (b1 - a1) / ES;
    if (tid < nhead + ntail) one(tid < nhead ? m0 + tid : m1 - ntail + (tid - nhead));   // fewer than 2 N lanes
    const uint4 *v = reinterpret_cast<const uint4 *>(base + a0);
    const int64_t nvec = (a1 - a0) / 16;
    // this lane's vectors are tid, tid + kBlock, ...: one position, stepped in order
    VecPos<K> pos;
    pos.init(wv, (uint32_t)(a0 / ES + (int64_t)tid * N), (uint32_t)(kBlock * N));
    auto take = [&](const uint4 &raw) {
        T x[N];
        double w[N];
        unpack16<T, BSWAP>(raw, x);
        vec_weights<N>(wv, pos, w);
        pos.advance(wv);
        acc.template add_n<N, M>(x, w, mk);
    };
    constexpr int U = 4;
    constexpr int64_t STEP = (int64_t)U * kBlock;
    const int64_t nsteps = nvec / STEP;
    if (nsteps > 0) {
        uint4 cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = ldg16(v + tid + u * kBlock);
        for (int64_t s = 0; s + 1 < nsteps; ++s) {
            // the next step's loads are in flight while this step is reduced
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = ldg16(v + (s + 1) * STEP + tid + u * kBlock);
#pragma unroll
            for (int u = 0; u < U; ++u) take(cur[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) take(cur[u]);
    }
    for (int64_t k = nsteps * STEP + tid; k < nvec; k += kBlock) take(ldg16(v + k));
}

// Shuffled layout, chunk elements [i0, i1); n = elements in the chunk.
template <typename T, bool BSWAP, int M, bool WL, int K>
__device__ __forceinline__ void ws_run_shuffled(const uint8_t *base, int64_t n, int64_t i0, int64_t i1, WsAcc &acc,
                                const MaskT<T> &mk, const WVec<WL, K> &wv) {
    constexpr int ES = sizeof(T);
    const int tid = threadIdx.x;
    const bool vec_ok = (((uintptr_t)base & 15) == 0) && ((n & 15) == 0);
    const int64_t g0 = (i0 + 15) & ~(int64_t)15, g1 = i1 & ~(int64_t)15;
    auto one = [&](int64_t i) {
        const T x = load_shuffled<T, BSWAP>(base, n, i);
        const double w = elem_weight(wv, i);
        acc.template add_n<1, M>(&x, &w, mk);
    };
    if (!vec_ok || g0 >= g1) {
        for (int64_t i = i0 + tid; i < i1; i += kBlock) one(i);
        return;
    }
    if (tid < (g0 - i0) + (i1 - g1)) one(tid < g0 - i0 ? i0 + tid : g1 + (tid - (g0 - i0)));   // fewer than 32 lanes
    const int64_t ng = (g1 - g0) / 16;
    VecPos<K> pos;
    pos.init(wv, (uint32_t)(g0 + (int64_t)tid * 16), (uint32_t)(kBlock * 16));
    for (int64_t g = tid; g < ng; g += kBlock) {
        const int64_t i = g0 + g * 16;
        uint4 pl[ES];
#pragma unroll
        for (int b = 0; b < ES; ++b) pl[b] = ldg16(reinterpret_cast<const uint4 *>(base + (int64_t)b * n + i));
        T x[16];
        double w[16];
        unshuffle16<T, BSWAP>(pl, x);
        vec_weights<16>(wv, pos, w);
        pos.advance(wv);
        acc.template add_n<16, M>(x, w, mk);
    }
}

template <typename T, bool SHUF, bool BSWAP, bool WL, int K>
__device__ __forceinline__ void ws_run(int mode, const uint8_t *base, int64_t n, int64_t i0, int64_t i1, WsAcc &acc,
                                       const MaskT<T> &mk, const WVec<WL, K> &wv) {
    if constexpr (!WL) {   // beyond the LDS path: one instantiation, which evaluates every mask rule at run time
        if constexpr (SHUF && sizeof(T) > 1) ws_run_shuffled<T, BSWAP, kMaskAll>(base, n, i0, i1, acc, mk, wv);
        else ws_run_plain<T, BSWAP, kMaskAll>(base, i0, i1, acc, mk, wv);
    } else if constexpr (SHUF && sizeof(T) > 1) {
        if (mode == 0) ws_run_shuffled<T, BSWAP, 0>(base, n, i0, i1, acc, mk, wv);
        else if (mode == kMaskRange) ws_run_shuffled<T, BSWAP, kMaskRange>(base, n, i0, i1, acc, mk, wv);
        else ws_run_shuffled<T, BSWAP, kMaskAll>(base, n, i0, i1, acc, mk, wv);
    } else {
        if (mode == 0) ws_run_plain<T, BSWAP, 0>(base, i0, i1, acc, mk, wv);
        else if (mode == kMaskRange) ws_run_plain<T, BSWAP, kMaskRange>(base, i0, i1, acc, mk, wv);
        else ws_run_plain<T, BSWAP, kMaskAll>(base, i0, i1, acc, mk, wv);
    }
}

// ---------------------------------------------------------------------------
// per-element walk: factors by dim, read from the pool
// ---------------------------------------------------------------------------
// Positions q0, q0 + stride, ... < n_pos over the dims in `dmask` (rc: the
// radix counter at q0), 4 loads in flight.  Dims outside dmask sit at chunk
// index kli[d] (already part of base_o); org: the chunk's row of origin.
template <typename T, bool SHUF>
__device__ __forceinline__ void ws_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t dmask,
                                        const Decomp &base_o, const int32_t *kli, const double *wpool,
                                        const int32_t *org, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                        int64_t stride, bool bsw, const MaskT<T> &mk, WsAcc &acc) {
    auto locate = [&](Decomp &o, double &w) {
        w = 1.0;
#pragma unroll
        for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
            if (d < r.ndim) {
                int64_t li = kli[d];
                if ((dmask >> d) & 1u) {
                    li = sel_index(s, r.pool, d, rc.idx[d]);
                    o.mem += li * r.cstride[d];
                    o.v[0] += (int64_t)rc.idx[d] * r.tab.stride[0][d];
                    o.v[1] += (int64_t)rc.idx[d] * r.tab.stride[1][d];
                }
                w *= wpool[org[d] + li];
            }
        }
    };
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp od[U];
        double w[U];
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            od[u] = base_o;
            locate(od[u], w[u]);
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od[u].mem, bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add(x[u], w[u], !all_masked(mk, r.tab, od[u], x[u]));
    }
    for (; q < n_pos; q += stride) {
        Decomp od = base_o;
        double w;
        locate(od, w);
        rc.advance();
        const T x = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od.mem, bsw);
        acc.add(x, w, !all_masked(mk, r.tab, od, x));
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_wsum_full(WsumArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, t = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    const int32_t *org = a.worigin + c * PYAS_MAX_DIMS;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    ws_mask_init(mk, r.mask);
    const bool tabs = r.tab.on[0] || r.tab.on[1];
    // One contiguous run?  From the innermost dim: whole dims, then one
    // unit-step range, then single indices.
    constexpr int NV = (SHUF && sizeof(T) > 1) ? 16 : 16 / (int)sizeof(T);   // elements per vector
    int64_t total = 1, m0 = 0, ext = 0;
    bool contig = !tabs, inner_full = true;
#pragma unroll
    for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
        if (d < r.ndim) {
            const int64_t cnt = s.cnt[d];
            total *= cnt;
            ext += r.shape[d];
            if (d == r.ndim - 1 && r.shape[d] < NV) contig = false;   // a vector would span 3 rows: walk
            if (s.step[d] == 0) contig = false;
            if (cnt != 1 && (!inner_full || s.step[d] != 1)) contig = false;
            m0 += (int64_t)s.start[d] * r.cstride[d];
            if (!(s.start[d] == 0 && s.step[d] == 1 && cnt == r.shape[d])) inner_full = false;
        }
    }
    int64_t e0, e1;
    tile_share(total, a.bpc, t, e0, e1);
    const int mode = mask_mode(a.masked, r.mask.flags);
    __shared__ double s_wt[kWLds];
    WsAcc acc;
    acc.init();
    if (contig && r.ndim <= 3 && ext <= kWLds) {       // (uniform)
        WVec<true, 3> wv;
        wvec_setup(wv, r, a.wpool, org, s_wt);
        __syncthreads();
        if (e0 < e1) {
            if (a.bswap) ws_run<T, SHUF, true>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk, wv);
            else ws_run<T, SHUF, false>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk, wv);
        }
    } else if (contig) {
        WVec<false, PYAS_MAX_DIMS> wv;
        wvec_setup(wv, r, a.wpool, org, s_wt);
        if (e0 < e1) {
            if (a.bswap) ws_run<T, SHUF, true>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk, wv);
            else ws_run<T, SHUF, false>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk, wv);
        }
    } else if (e0 + threadIdx.x < e1) {
        const uint32_t all = (1u << r.ndim) - 1u;
        RadixCounter rc;
        rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
        const Decomp zero{0, {0, 0}};
        const int32_t kli[PYAS_MAX_DIMS] = {0, 0, 0, 0, 0, 0, 0, 0};
        ws_walk<T, SHUF>(r, base, s, all, zero, kli, a.wpool, org, rc, e0 + threadIdx.x, e1, kBlock, a.bswap, mk,
                         acc);
    }
    rec_store_full<WsumMerge>(acc, a, c);
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
// (ws_keep of pyas_wvec.hpp: output o's kept coordinates)
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_wsum_axes(WsumArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    const int32_t *org = a.worigin + c * PYAS_MAX_DIMS;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    ws_mask_init(mk, r.mask);
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep, n_red;
    axes_extents(s, r.ndim, red, n_keep, n_red);
    pyas_wsum *out = a.out + a.out_offsets[c];
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            WsAcc acc;
            acc.init();
            if (n_red > 0) {
                Decomp bo{0, {0, 0}};
                int32_t kli[PYAS_MAX_DIMS];
                ws_keep(r, s, keep, o, bo, kli);
                RadixCounter rc;
                rc.init(s, r.ndim, red, 0, 1);
                ws_walk<T, SHUF>(r, base, s, red, bo, kli, a.wpool, org, rc, 0, n_red, 1, a.bswap, mk, acc);
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            WsAcc acc;
            acc.init();
            if (lane < n_red) {
                Decomp bo{0, {0, 0}};
                int32_t kli[PYAS_MAX_DIMS];
                ws_keep(r, s, keep, o, bo, kli);
                RadixCounter rc;
                rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                ws_walk<T, SHUF>(r, base, s, red, bo, kli, a.wpool, org, rc, lane, n_red, kWave, a.bswap, mk, acc);
            }
            pyas_wsum p = acc.finish();
            rec_wave_merge<pyas_wsum, WsumMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

hipError_t launch_wsum_full(int dtype, const WsumArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_wsum_full), a, shuf, grid, 0, st)
}

hipError_t launch_wsum_axes(int dtype, const WsumArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_wsum_axes), a, shuf, grid, 0, st)
}

hipError_t launch_wsum_tiles(const pyas_wsum *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                             pyas_wsum *out, hipStream_t st) {
    return launch_rec_tiles<pyas_wsum, WsumMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

hipError_t launch_wsum_segments(const pyas_wsum *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_wsum *out, hipStream_t st) {
    return launch_rec_segments<pyas_wsum, WsumMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_wsum_grid(const pyas_wsum *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                            pyas_wsum *out, hipStream_t st) {
    return launch_rec_grid<pyas_wsum, WsumMerge>(in, g, n_out, n_layers, out, st);
}

}  // namespace pyas
