// pyas_trend.hip — least-squares trend kernels behind Active.trend
// (pyas_trend_axes, pyas_trend_cols and pyas_trend_finalize of include/pyas.h).
//
// The co-moment record of pyas_comoments.hip with x a coordinate instead of a
// second stored variable: x = pool[origin[c] + i], i the element's index inside
// chunk c along the coordinate's dim, y the data value.  A lane accumulates as
// CoAcc does (shifts from its first counted pair, sums in f64 with FMA, masked
// elements excluded by select) and finishes to a pyas_comoments record;
// everything above a lane merges records with ComomMerge in a fixed order, so a
// result is bit-identical from run to run.
//
// k_trend_cols : the dense path.  Unit-step box queries whose reduced dims are a
//                leading prefix of the dims.  A workgroup owns 256 items of one
//                column of chunks (the chunks that share their kept dims' chunk
//                coordinates); an item is kTrendV = 4 consecutive outputs along
//                the innermost dim, aligned to 4 elements of the chunk row, so a
//                wave reads 256 consecutive elements of every row.  A lane walks
//                its 4 outputs through every row of every chunk layer of the
//                column in increasing index order and writes 4 finished records:
//                the layers fold inside the lane, no per-chunk record is written
//                and nothing is merged.  Per pass the workgroup stages up to
//                kTrendRows rows' element offsets and coordinates in LDS (the
//                coordinate of a row is one LDS broadcast, not a load per
//                element); 4 rows are fetched at a time and, for types below 8
//                bytes, the next 4 rows' loads are in flight while these are
//                accumulated.  An item wholly inside the selection of a chunk
//                whose rows are aligned takes one load of 4 elements (16 B for
//                4-byte types, 2 x 16 B for 8-byte types, 8 B and 4 B for 2- and
//                1-byte types; a shuffled chunk one 4-B load per byte plane);
//                items cut by the box and chunks whose rows are not a multiple of
//                4 elements load per element under a predicate, so padding and
//                unselected elements are never read.  Templated on the dtype and
//                shuffled-or-not (18 kernels); byte order is a run-time flag
//                behind one template switch, the mask mode a run-time switch.
// k_trend_axes : everything else (strides, index lists, vector mask tables,
//                reduced dims that are not a prefix, every dim reduced): the
//                k_comoments_axes walk with y's load replaced by the coordinate
//                look-up, one record per chunk output.  Correct, no speed
//                target.  Templated on the dtype only (10 kernels).
// k_trend_finalize : slope or intercept and the mask byte of n records.
#include <hip/hip_runtime.h>

#include "pyas_comoments.hpp"   // ComomMerge, CoAcc
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode, rec_wave_merge

namespace pyas {

// ---------------------------------------------------------------------------
// k_trend_axes: the per-element walk
// ---------------------------------------------------------------------------
constexpr int kTrendRoff = 2048;   // reduced positions kept in LDS (int32 offsets + f64 coordinates, 24 KiB)

struct TrSide {
    const uint8_t *base;
    const double *cx;      // the chunk's coordinates: cx[i], i the index inside the chunk along cdim
    int cdim;
    bool shuf, bsw;
};

// the index inside the chunk along cdim at the radix counter's position (no
// register array is indexed by a run-time value)
__device__ __forceinline__ int64_t tr_coord_index(const Sel &s, const int32_t *pool, int cdim,
                                                  const RadixCounter &rc) {
    int64_t li = 0;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d == cdim) li = sel_index(s, pool, d, rc.idx[d]);
    return li;
}

// Positions q0, q0 + stride, ... < n_pos over the dims in `dmask` (rc: the
// radix counter at q0; cdim is one of them); bo: the kept dims' part.
template <typename T>
__device__ __forceinline__ void tr_walk(const ReduceArgs &r, const TrSide &ts, const Sel &s, uint32_t dmask,
                                        const Decomp &bo, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                        int64_t stride, const MaskT<T> &mk, CoAcc &acc) {
    constexpr int U = 2;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp o[U];
        double x[U];
        T y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            o[u] = bo;
            rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, o[u]);
            x[u] = ts.cx[tr_coord_index(s, r.pool, ts.cdim, rc)];
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) y[u] = load_elem_rt<T>(ts.base, r.chunk_elems, o[u].mem, ts.shuf, ts.bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one(x[u], (double)y[u], !all_masked(mk, r.tab, o[u], y[u]));
    }
    for (; q < n_pos; q += stride) {
        Decomp o = bo;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, o);
        const double x = ts.cx[tr_coord_index(s, r.pool, ts.cdim, rc)];
        rc.advance();
        const T y = load_elem_rt<T>(ts.base, r.chunk_elems, o.mem, ts.shuf, ts.bsw);
        acc.add_one(x, (double)y, !all_masked(mk, r.tab, o, y));
    }
}

// The same walk with the reduced positions' element offsets and coordinates
// already in LDS (no vector mask tables).
template <typename T>
__device__ __forceinline__ void tr_walk_lds(const ReduceArgs &r, const TrSide &ts, const int32_t *roff,
                                            const double *rx, int64_t base_mem, int64_t q0, int64_t n_pos,
                                            int64_t stride, const MaskT<T> &mk, CoAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        T y[U];
#pragma unroll
        for (int u = 0; u < U; ++u)
            y[u] = load_elem_rt<T>(ts.base, r.chunk_elems, base_mem + roff[q + u * stride], ts.shuf, ts.bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one(rx[q + u * stride], (double)y[u], !mk.masked(y[u]));
    }
    for (; q < n_pos; q += stride) {
        const T y = load_elem_rt<T>(ts.base, r.chunk_elems, base_mem + roff[q], ts.shuf, ts.bsw);
        acc.add_one(rx[q], (double)y, !mk.masked(y));
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_trend_axes(TrendArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const TrSide ts{r.data + r.offsets[c], a.cpool + a.corigin[c], a.cdim, a.shuf, a.bswap};
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep = 1, n_red = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
        if (d < r.ndim) {
            if ((red >> d) & 1u) n_red *= s.cnt[d];
            else n_keep *= s.cnt[d];
        }
    }
    pyas_comoments *out = a.out + (a.out_offsets ? a.out_offsets[c] : c);
    // the reduced positions' offsets and coordinates, once per workgroup, when they fit
    __shared__ int32_t s_roff[kTrendRoff];
    __shared__ double s_rx[kTrendRoff];
    const bool mapped = !(r.tab.on[0] || r.tab.on[1]) && n_red <= kTrendRoff;   // uniform
    if (mapped) {
        for (int64_t q = threadIdx.x; q < n_red; q += kBlock) {
            int64_t e = q, mem = 0, li_c = 0;
#pragma unroll
            for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
                if (d < r.ndim && ((red >> d) & 1u)) {
                    const int64_t cd = s.cnt[d];
                    const int64_t qq = e / cd, k = e - qq * cd;
                    e = qq;
                    const int64_t li = sel_index(s, r.pool, d, k);
                    mem += li * r.cstride[d];
                    if (d == a.cdim) li_c = li;
                }
            }
            s_roff[q] = (int32_t)mem;   // |offset| < chunk elements < 2^31
            s_rx[q] = ts.cx[li_c];
        }
        __syncthreads();
    }
    auto kept_part = [&](int64_t o, Decomp &bo) {
        bo = Decomp{0, {0, 0}};
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
    };
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            CoAcc acc;
            acc.init();
            if (n_red > 0) {
                Decomp bo;
                kept_part(o, bo);
                if (mapped) {
                    tr_walk_lds<T>(r, ts, s_roff, s_rx, bo.mem, 0, n_red, 1, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, 0, 1);
                    tr_walk<T>(r, ts, s, red, bo, rc, 0, n_red, 1, mk, acc);
                }
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            CoAcc acc;
            acc.init();
            if (lane < n_red) {
                Decomp bo;
                kept_part(o, bo);
                if (mapped) {
                    tr_walk_lds<T>(r, ts, s_roff, s_rx, bo.mem, lane, n_red, kWave, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                    tr_walk<T>(r, ts, s, red, bo, rc, lane, n_red, kWave, mk, acc);
                }
            }
            pyas_comoments p = acc.finish();
            rec_wave_merge<pyas_comoments, ComomMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// k_trend_cols: the dense column walk
// ---------------------------------------------------------------------------
#ifndef PYAS_TREND_ATTR
#define PYAS_TREND_ATTR
#endif
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct TrRows {
    static constexpr int U = 4;
    T v[U][kTrendV];
};

// rows q .. q + U - 1 (those below nq) into y
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void tr_fetch(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                         const int32_t *roff, int q, int nq, TrRows<T> &y) {
    constexpr int U = TrRows<T>::U, V = kTrendV;
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < V; ++k) y.v[u][k] = (T)0;
        if (q + u < nq) {   // (uniform)
            const int64_t i = kmem + roff[q + u];
            if (vec4) {
                T t[V];
                tr_load4<T, SHUF, BSW>(base, n, i, t);
#pragma unroll
                for (int k = 0; k < V; ++k) y.v[u][k] = t[k];
            } else {
#pragma unroll
                for (int k = 0; k < V; ++k)
                    if (in[k]) y.v[u][k] = load_elem<T, SHUF, BSW>(base, n, i + k);
            }
        }
    }
}

// FIRST: some output of the wave still looks for its shifts
template <typename T, int M, bool FIRST>
__device__ __forceinline__ void tr_consume(const TrRows<T> &y, const bool *in, const double *cx, int q, int nq,
                                           const MaskT<T> &mk, CoAcc *acc) {
    constexpr int U = TrRows<T>::U, V = kTrendV;
#pragma unroll
    for (int u = 0; u < U; ++u) {
        if (q + u < nq) {   // (uniform)
            const double x = cx[q + u];
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const T v = y.v[u][k];
                const bool ok = in[k] && (M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v));
                if constexpr (FIRST) acc[k].add_one(x, (double)v, ok);
                else acc[k].add_next(x, (double)v, ok);
            }
        }
    }
}

// nq staged rows (roff: their element offsets, cx: their coordinates) into the
// lane's 4 accumulators; `in`: which of the 4 outputs are selected, vec4: all
// of them and the chunk's rows are aligned.  Register double buffer: the next
// U rows' loads are in flight while these U rows are accumulated.  (8-byte
// types keep one buffer: a second one takes them past 256 VGPRs, to one wave
// per SIMD.)
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void tr_rows(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                        const int32_t *roff, const double *cx, int nq, const MaskT<T> &mk,
                                        CoAcc *acc) {
    constexpr int U = TrRows<T>::U, V = kTrendV;
    constexpr bool DB = sizeof(T) < 8;
    TrRows<T> cur, nxt;
    if constexpr (DB) tr_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if constexpr (DB) {
            if (q + U < nq) tr_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q + U, nq, nxt);   // (uniform)
        } else {
            tr_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q, nq, cur);
        }
        bool first = false;
#pragma unroll
        for (int k = 0; k < V; ++k) first |= in[k] && acc[k].n == 0;
        // once every output of the wave has its shifts they are no longer looked for
        if (__builtin_expect(__ballot(first) != 0, 0)) tr_consume<T, M, true>(cur, in, cx, q, nq, mk, acc);
        else tr_consume<T, M, false>(cur, in, cx, q, nq, mk, acc);
        if constexpr (DB) cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void tr_rows_m(int mode, const uint8_t *base, int64_t n, int64_t kmem, bool vec4,
                                          const bool *in, const int32_t *roff, const double *cx, int nq,
                                          const MaskT<T> &mk, CoAcc *acc) {
    if (mode == 0) tr_rows<T, SHUF, BSW, 0>(base, n, kmem, vec4, in, roff, cx, nq, mk, acc);
    else if (mode == kMaskRange) tr_rows<T, SHUF, BSW, kMaskRange>(base, n, kmem, vec4, in, roff, cx, nq, mk, acc);
    else tr_rows<T, SHUF, BSW, kMaskAll>(base, n, kmem, vec4, in, roff, cx, nq, mk, acc);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) PYAS_TREND_ATTR void k_trend_cols(TrendColsArgs a) {
    constexpr int V = kTrendV, ES = sizeof(T);
    const ReduceArgs &r = a.r;
    const int nd = r.ndim, P = a.P, L = nd - 1;
    const int64_t col = (int64_t)blockIdx.x / a.bpc, sb = (int64_t)blockIdx.x % a.bpc;
    // The kept dims' selection is the same in every layer of the column: read
    // it from layer 0 (chunk `col`).
    Sel s0;
    load_sel(s0, r.sel, col, nd, r.shape);
    int64_t KO = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d >= P && d < L) KO *= s0.cnt[d];
    int32_t st = 0, cn = 0;   // the innermost dim's selection
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d == L) {
            st = s0.start[d];
            cn = s0.cnt[d];
        }
    const int32_t g0 = st / V;
    const int32_t G = cn > 0 ? (st + cn - 1) / V - g0 + 1 : 0;   // groups of 4 chunk elements the row's selection touches
    const int64_t n_items = KO * G;
    if (sb * kBlock >= n_items) return;   // (uniform) nothing for this workgroup
    const int64_t item = sb * kBlock + threadIdx.x;
    const bool live = item < n_items;
    int64_t ko = live ? item / G : 0;
    const int32_t g = live ? (int32_t)(item - ko * G) : 0;
    const int32_t i0 = (g0 + g) * V;   // the innermost chunk index of the lane's first output
    bool in[V], full = true;
#pragma unroll
    for (int k = 0; k < V; ++k) {
        in[k] = live && i0 + k >= st && i0 + k < st + cn;
        full = full && in[k];
    }
    // the kept dims' part: chunk memory and the final output index of output 0
    int64_t kmem = i0, fidx = 0;
    {
        int64_t rest = col, cs = 1;
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (d < nd && d >= P) {
                const int64_t nc = a.n_coords[d];
                const int64_t ad = rest % nc;
                rest /= nc;
                // A unit-step box: every chunk but the first along d starts at 0 and
                // the first runs to the chunk's end, so the column's first output
                // position along d follows from the first chunk's start.
                const int64_t first = col - ad * cs;
                const int64_t st0 = r.sel ? r.sel[(first * PYAS_MAX_DIMS + d) * 3] : 0;
                const int64_t ostart = ad == 0 ? 0 : (r.shape[d] - st0) + (ad - 1) * r.shape[d];
                cs *= nc;
                if (d == L) {
                    fidx += (ostart + (i0 - st)) * a.ostride[d];
                } else {
                    const int64_t cd = s0.cnt[d];
                    const int64_t qq = ko / cd, k = ko - qq * cd;
                    ko = qq;
                    kmem += (s0.start[d] + k) * r.cstride[d];
                    fidx += (ostart + k) * a.ostride[d];
                }
            }
        }
    }
    MaskT<T> mk;
    mk.init(r.mask);
    const int mode = mask_mode(a.masked, r.mask.flags);
    // 4-element loads: every row of the chunk starts at a multiple of 4 elements
    // (and so does every byte plane of a shuffled chunk)
    constexpr int64_t kAlign = (SHUF && ES > 1) ? 4 : (ES * V < 16 ? ES * V : 16);
    const bool vec_geom = (r.shape[L] % V) == 0;
    __shared__ int32_t s_roff[kTrendRows];
    __shared__ double s_cx[kTrendRows];
    CoAcc acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k].init();
    for (int64_t l = 0; l < a.n_layers; ++l) {
        const int64_t c = l * a.n_cols + col;
        const uint8_t *base = r.data + r.offsets[c];
        const double *cx = a.cpool + a.corigin[c];
        // the reduced dims' selection of this layer
        int32_t rst[PYAS_MAX_DIMS], rcn[PYAS_MAX_DIMS];
        int64_t R = 1;
#pragma unroll
        for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
            rst[d] = 0;
            rcn[d] = 1;
            if (d < P) {
                if (r.sel) {
                    const int32_t *p = r.sel + (c * PYAS_MAX_DIMS + d) * 3;
                    rst[d] = p[0];
                    rcn[d] = p[2];
                } else {
                    rcn[d] = (int32_t)r.shape[d];
                }
                R *= rcn[d];
            }
        }
        const bool vec4 = full && vec_geom && (((uintptr_t)base & (kAlign - 1)) == 0);
        for (int64_t t0 = 0; t0 < R; t0 += kTrendRows) {
            const int nq = (int)(R - t0 < kTrendRows ? R - t0 : kTrendRows);
            __syncthreads();   // the previous pass has been read
            for (int q = threadIdx.x; q < nq; q += kBlock) {
                int64_t e = t0 + q, mem = 0, li_c = 0;
#pragma unroll
                for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
                    if (d < P) {
                        const int64_t cd = rcn[d];
                        const int64_t qq = e / cd, k = e - qq * cd;
                        e = qq;
                        const int64_t li = rst[d] + k;
                        mem += li * r.cstride[d];
                        if (d == a.cdim) li_c = li;
                    }
                }
                s_roff[q] = (int32_t)mem;   // < chunk elements < 2^31
                s_cx[q] = cx[li_c];
            }
            __syncthreads();
            if (live) {
                if (a.bswap) tr_rows_m<T, SHUF, true>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, s_cx, nq, mk, acc);
                else tr_rows_m<T, SHUF, false>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, s_cx, nq, mk, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (in[k]) a.out[fidx + k * a.ostride[L]] = acc[k].finish();
}

// ---------------------------------------------------------------------------
// k_trend_finalize
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_trend_finalize(const pyas_comoments *in, int64_t n, int32_t what,
                                                           double *value, uint8_t *masked) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const pyas_comoments p = in[i];
    const double slope = p.cxy / p.m2_x;   // 0 / 0 (one element, equal coordinates): NaN
    const double v = what == 0 ? slope : __builtin_fma(-slope, p.mean_x, p.mean_y);
    const bool empty = p.count == 0;
    value[i] = empty ? 0.0 : v;
    masked[i] = empty ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_tr_axes_t(const TrendArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_trend_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_trend_axes(int dtype, const TrendArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_tr_axes_t, a, grid, st)
}

hipError_t launch_trend_cols(int dtype, const TrendColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_trend_cols), a, shuf, grid, 0, st)
}

hipError_t launch_trend_finalize(const pyas_comoments *in, int64_t n, int32_t what, double *value, uint8_t *masked,
                                 hipStream_t st) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_trend_finalize, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, what, value, masked);
    return hipGetLastError();
}

}  // namespace pyas
