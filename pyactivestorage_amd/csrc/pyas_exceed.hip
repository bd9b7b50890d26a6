// pyas_exceed.hip — conditional-reduction kernels behind Active.exceed
// (pyas_exceed_axes, pyas_exceed_cols, the two exceed combines and
// pyas_exceed_finalize of include/pyas.h).
//
// A position is true when its element is unmasked and float64(x) op t holds, t
// the threshold of the position's output: one scalar, or an entry of a field
// with one threshold per output (ExcTest: values[origin[c] + sum local[d] *
// stride[d]]).  The record (pyas_exceed) counts the unmasked and the true
// positions and adds, over the true ones, x and |x - t| in f64.  Per lane:
// n, n_true, sum, excess in registers; masked and false elements are excluded
// by select (never multiplied by 0).  lt / le compare -x against -t, so the
// excess term is the one subtraction (-x) - (-t) = t - x.  Everything above a
// lane merges records by addition in a fixed order, so a result is
// bit-identical from run to run.
//
// k_exceed_full : every dim reduced (scalar threshold), one workgroup per
//                 (chunk, tile).  A whole chunk or a selection that is one
//                 contiguous run streams 16-B loads (stat_run); anything else
//                 walks per element (stat_walk).
// k_exceed_axes : partial axes, one record per kept output, any selection and
//                 mask.  Innermost dim kept: a lane per output; innermost dim
//                 reduced: a wave per output.  The output's threshold is loaded
//                 once per output.
// k_exceed_cols : the dense path, k_trend_cols (pyas_trend.hip) without the
//                 coordinate.  Unit-step box queries whose reduced dims are a
//                 leading prefix of the dims.  A lane owns kTrendV = 4
//                 consecutive outputs along the innermost dim, loads their 4
//                 thresholds once and walks every row of every chunk layer of
//                 its column; it writes 4 finished records and merges nothing.
//                 Staging, loads and predicates as in k_trend_cols; the
//                 accumulator is small, so every type keeps the register double
//                 buffer.
// k_exceed_finalize : one stat of n records (8 bytes) and the mask byte.
// The three data kernels are templated on the dtype and shuffled-or-not only;
// byte order, mask rules and selection kind are run-time branches.
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // the tile / segment / grid combines
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // the runs, the walk, the offset map, the record merges

namespace pyas {

// ---------------------------------------------------------------------------
// the record
// ---------------------------------------------------------------------------
struct ExcMerge {
    // a then b (the order matters to the last bit of the sums, so every caller fixes it)
    static __device__ __forceinline__ pyas_exceed merged(const pyas_exceed &a, const pyas_exceed &b) {
        pyas_exceed r;
        r.n = a.n + b.n;
        r.n_true = a.n_true + b.n_true;
        r.sum = a.sum + b.sum;
        r.excess = a.excess + b.excess;
        return r;
    }
    static __device__ __forceinline__ pyas_exceed shfl_xor(const pyas_exceed &p, int m) {
        pyas_exceed q;
        q.n = pyas::shfl_xor(p.n, m);
        q.n_true = pyas::shfl_xor(p.n_true, m);
        q.sum = pyas::shfl_xor(p.sum, m);
        q.excess = pyas::shfl_xor(p.excess, m);
        return q;
    }
};

// One output's positions.  thr: the output's threshold as it is compared
// (negated when neg).  A lane counts fewer than 2^32 positions.
struct ExcAcc {
    double thr, sum, exc;
    uint32_t n, nt;
    bool neg, incl;
    __device__ __forceinline__ void init(double threshold, bool neg_, bool incl_) {
        thr = threshold; sum = 0.0; exc = 0.0; n = 0; nt = 0;
        neg = neg_; incl = incl_;
    }
    // one element; ok = selected and unmasked
    __device__ __forceinline__ void add_one(double x, bool ok) {
        const double xs = neg ? -x : x;
        const bool tr = ok & ((xs > thr) | (incl & (xs == thr)));   // a NaN on either side: false
        n += ok ? 1u : 0u;
        nt += tr ? 1u : 0u;
        sum = tr ? sum + x : sum;
        exc = tr ? exc + (xs - thr) : exc;
    }
    // N values; M: mask mode (0 none, kMaskRange, kMaskAll)
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const MaskT<T> &mk) {
#pragma unroll
        for (int k = 0; k < N; ++k) add_one((double)x[k], M ? !mk.template masked_m<M ? M : kMaskAll>(x[k]) : true);
    }
    // N values; ok[k]: x[k] is selected and unmasked
    template <int N, typename T>
    __device__ __forceinline__ void add(const T *x, const bool *ok) {
#pragma unroll
        for (int k = 0; k < N; ++k) add_one((double)x[k], ok[k]);
    }
    __device__ __forceinline__ pyas_exceed finish() const {
        pyas_exceed p;
        p.n = (int64_t)n;
        p.n_true = (int64_t)nt;
        p.sum = sum;
        p.excess = exc;
        return p;
    }
};

// The threshold, as it is compared, of output o (C order over the kept selected
// dims `keep`) of chunk c.
__device__ __forceinline__ double exc_threshold(const ExcTest &t, const ReduceArgs &r, const Sel &s, uint32_t keep,
                                                int64_t c, int64_t o) {
    if (!t.values) return t.threshold;
    int64_t e = o, off = t.origin[c];
#pragma unroll
    for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
        if (d < r.ndim && ((keep >> d) & 1u)) {
            const int64_t cd = s.cnt[d];
            const int64_t q = e / cd, k = e - q * cd;
            e = q;
            off += sel_index(s, r.pool, d, k) * t.stride[d];
        }
    }
    const double v = t.values[off];
    return t.neg ? -v : v;
}

// stat_walk with the reduced positions' element offsets already in LDS (no
// vector mask tables): per element one LDS read, one add, one load.
constexpr int kExcRoff = 4096;   // reduced positions kept in LDS (int32, 16 KiB)
template <typename T, bool SHUF>
__device__ __forceinline__ void exc_walk_lds(const uint8_t *base, int64_t chunk_elems, const int32_t *roff,
                                             int64_t base_mem, int64_t q0, int64_t n_pos, int64_t stride, bool bsw,
                                             const MaskT<T> &mk, ExcAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        T x[U];
        bool ok[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = load_elem_bsw<T, SHUF>(base, chunk_elems, base_mem + roff[q + u * stride], bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) ok[u] = !mk.masked(x[u]);
        acc.template add<U>(x, ok);
    }
    for (; q < n_pos; q += stride) {
        const T x = load_elem_bsw<T, SHUF>(base, chunk_elems, base_mem + roff[q], bsw);
        const bool ok = !mk.masked(x);
        acc.template add<1>(&x, &ok);
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_exceed_full(ExceedArgs a) {
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
    int64_t e0, e1;
    tile_share(total, a.bpc, t, e0, e1);
    ExcAcc acc;
    acc.init(a.t.threshold, a.t.neg, a.t.incl);
    if (e0 < e1) {
        if (contig) {
            const int mode = mask_mode(a.masked, r.mask.flags);
            if (a.bswap) stat_run<T, SHUF, true>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
            else stat_run<T, SHUF, false>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
        } else if (e0 + threadIdx.x < e1) {
            const uint32_t all = (1u << r.ndim) - 1u;
            RadixCounter rc;
            rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
            const Decomp zero{0, {0, 0}};
            stat_walk<T, SHUF>(r, base, s, all, zero, rc, e0 + threadIdx.x, e1, kBlock, a.bswap, mk, acc);
        }
    }
    rec_store_full<ExcMerge>(acc, a, c);
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_exceed_axes(ExceedArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep, n_red;
    axes_extents(s, r.ndim, red, n_keep, n_red);
    // the reduced positions' offsets, once per workgroup, when they fit
    __shared__ int32_t s_roff[kExcRoff];
    const bool mapped = !(r.tab.on[0] || r.tab.on[1]) && n_red <= kExcRoff;   // uniform
    if (mapped) stage_roff(r, s, red, n_red, s_roff);
    pyas_exceed *out = a.out + a.out_offsets[c];
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            ExcAcc acc;
            acc.init(exc_threshold(a.t, r, s, keep, c, o), a.t.neg, a.t.incl);
            if (n_red > 0) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    exc_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, 0, n_red, 1, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, 0, 1);
                    stat_walk<T, SHUF>(r, base, s, red, bo, rc, 0, n_red, 1, a.bswap, mk, acc);
                }
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            ExcAcc acc;
            acc.init(exc_threshold(a.t, r, s, keep, c, o), a.t.neg, a.t.incl);
            if (lane < n_red) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    exc_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, lane, n_red, kWave, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                    stat_walk<T, SHUF>(r, base, s, red, bo, rc, lane, n_red, kWave, a.bswap, mk, acc);
                }
            }
            pyas_exceed p = acc.finish();
            rec_wave_merge<pyas_exceed, ExcMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// k_exceed_cols: the dense column walk
// ---------------------------------------------------------------------------
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct ExcRows {
    static constexpr int U = 4;
    T v[U][kTrendV];
};

// rows q .. q + U - 1 (those below nq) into y
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void exc_fetch(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                          const int32_t *roff, int q, int nq, ExcRows<T> &y) {
    constexpr int U = ExcRows<T>::U, V = kTrendV;
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

// nq staged rows (roff: their element offsets) into the lane's 4 accumulators;
// `in`: which of the 4 outputs are selected, vec4: all of them and the chunk's
// rows are aligned.  Register double buffer: the next U rows' loads are in
// flight while these U rows are accumulated.
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void exc_rows(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                         const int32_t *roff, int nq, const MaskT<T> &mk, ExcAcc *acc) {
    constexpr int U = ExcRows<T>::U, V = kTrendV;
    ExcRows<T> cur, nxt;
    exc_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if (q + U < nq) exc_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q + U, nq, nxt);   // (uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q + u < nq) {   // (uniform)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const T v = cur.v[u][k];
                    acc[k].add_one((double)v, in[k] && (M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v)));
                }
            }
        }
        cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void exc_rows_m(int mode, const uint8_t *base, int64_t n, int64_t kmem, bool vec4,
                                           const bool *in, const int32_t *roff, int nq, const MaskT<T> &mk,
                                           ExcAcc *acc) {
    if (mode == 0) exc_rows<T, SHUF, BSW, 0>(base, n, kmem, vec4, in, roff, nq, mk, acc);
    else if (mode == kMaskRange) exc_rows<T, SHUF, BSW, kMaskRange>(base, n, kmem, vec4, in, roff, nq, mk, acc);
    else exc_rows<T, SHUF, BSW, kMaskAll>(base, n, kmem, vec4, in, roff, nq, mk, acc);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_exceed_cols(ExceedColsArgs a) {
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
    // the kept dims' part: chunk memory, the final output index and the field
    // offset of output 0 (as k_trend_cols: a unit-step box, so a column's first
    // output position along d follows from the first chunk's start)
    int64_t kmem = i0, fidx = 0, toff = 0, tstr = 0;
    {
        int64_t rest = col, cs = 1;
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (d < nd && d >= P) {
                const int64_t nc = a.n_coords[d];
                const int64_t ad = rest % nc;
                rest /= nc;
                const int64_t first = col - ad * cs;
                const int64_t st0 = r.sel ? r.sel[(first * PYAS_MAX_DIMS + d) * 3] : 0;
                const int64_t ostart = ad == 0 ? 0 : (r.shape[d] - st0) + (ad - 1) * r.shape[d];
                cs *= nc;
                if (d == L) {
                    fidx += (ostart + (i0 - st)) * a.ostride[d];
                    toff += i0 * a.t.stride[d];
                    tstr = a.t.stride[d];
                } else {
                    const int64_t cd = s0.cnt[d];
                    const int64_t qq = ko / cd, k = ko - qq * cd;
                    ko = qq;
                    kmem += (s0.start[d] + k) * r.cstride[d];
                    fidx += (ostart + k) * a.ostride[d];
                    toff += (s0.start[d] + k) * a.t.stride[d];
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
    // the 4 outputs' thresholds, once (an unselected output's is never compared)
    ExcAcc acc[V];
    {
        const double *tv = a.t.values ? a.t.values + a.t.origin[col] + toff : nullptr;
#pragma unroll
        for (int k = 0; k < V; ++k) {
            double th = a.t.threshold;
            if (tv) {
                const double v = in[k] ? tv[k * tstr] : 0.0;
                th = a.t.neg ? -v : v;
            }
            acc[k].init(th, a.t.neg, a.t.incl);
        }
    }
    for (int64_t l = 0; l < a.n_layers; ++l) {
        const int64_t c = l * a.n_cols + col;
        const uint8_t *base = r.data + r.offsets[c];
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
                int64_t e = t0 + q, mem = 0;
#pragma unroll
                for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
                    if (d < P) {
                        const int64_t cd = rcn[d];
                        const int64_t qq = e / cd, k = e - qq * cd;
                        e = qq;
                        mem += (rst[d] + k) * r.cstride[d];
                    }
                }
                s_roff[q] = (int32_t)mem;   // < chunk elements < 2^31
            }
            __syncthreads();
            if (live) {
                if (a.bswap) exc_rows_m<T, SHUF, true>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, acc);
                else exc_rows_m<T, SHUF, false>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (in[k]) a.out[fidx + k * a.ostride[L]] = acc[k].finish();
}

// ---------------------------------------------------------------------------
// k_exceed_finalize
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_exceed_finalize(const pyas_exceed *in, int64_t n, int32_t stat,
                                                            const uint8_t *thr_masked, void *value,
                                                            uint8_t *masked) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const pyas_exceed p = in[i];
    const bool tm = thr_masked && thr_masked[i] != 0;
    const bool bad = tm || (stat == PYAS_EXCEED_MEAN ? p.n_true == 0 : p.n == 0);
    if (stat == PYAS_EXCEED_COUNT) {
        static_cast<int64_t *>(value)[i] = bad ? 0 : p.n_true;
    } else {
        const double v = stat == PYAS_EXCEED_FRACTION ? (double)p.n_true / (double)p.n
                         : stat == PYAS_EXCEED_SUM    ? p.sum
                         : stat == PYAS_EXCEED_MEAN   ? p.sum / (double)p.n_true
                                                      : p.excess;
        static_cast<double *>(value)[i] = bad ? 0.0 : v;
    }
    masked[i] = bad ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_exceed_full(int dtype, const ExceedArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_exceed_full), a, shuf, grid, 0, st)
}

hipError_t launch_exceed_axes(int dtype, const ExceedArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_exceed_axes), a, shuf, grid, 0, st)
}

hipError_t launch_exceed_cols(int dtype, const ExceedColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_exceed_cols), a, shuf, grid, 0, st)
}

// the combines: pyas_records.hpp over the record and ExcMerge
hipError_t launch_exceed_tiles(const pyas_exceed *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                               pyas_exceed *out, hipStream_t st) {
    return launch_rec_tiles<pyas_exceed, ExcMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

hipError_t launch_exceed_segments(const pyas_exceed *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                  pyas_exceed *out, hipStream_t st) {
    return launch_rec_segments<pyas_exceed, ExcMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_exceed_grid(const pyas_exceed *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                              pyas_exceed *out, hipStream_t st) {
    return launch_rec_grid<pyas_exceed, ExcMerge>(in, g, n_out, n_layers, out, st);
}

hipError_t launch_exceed_finalize(const pyas_exceed *in, int64_t n, int32_t stat, const uint8_t *thr_masked,
                                  void *value, uint8_t *masked, hipStream_t st) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_exceed_finalize, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, stat, thr_masked, value,
                       masked);
    return hipGetLastError();
}

}  // namespace pyas
