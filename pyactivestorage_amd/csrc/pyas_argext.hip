// pyas_argext.hip — arg-extreme kernels behind Active.argmax / Active.argmin
// (pyas_argext_axes, pyas_argext_cols, the two argext combines and
// pyas_argext_finalize of include/pyas.h).
//
// The record (pyas_argext) is the winning element of a set of unmasked
// elements along one dim: its value in the data's class, its global index
// along the dim and the count of unmasked elements.  One element beats another
// when it is a NaN and the other is not, or when neither is a NaN and it is
// larger (argmax) / smaller (argmin) in the variable's own type; among equals
// (two NaNs, -0.0 and +0.0 included) the smaller index wins.  That order is
// total, so the merge is associative and commutative and every path gives the
// same record.
//
// Max and min are one code path: a kernel compares keys, key = x for argmax
// and -x (floats) or ~x (integers: the order reversed without overflow) for
// argmin, and the record holds the untouched value (both maps are their own
// inverse, bit for bit).
//
// k_argext_cols : the dense path, k_spell_cols (pyas_spell.hip) with another
//                accumulator.  Unit-step box queries with dim 0 the one reduced
//                dim.  A lane owns kTrendV = 4 consecutive outputs along the
//                innermost dim and walks every row of every chunk layer of its
//                column in increasing index order, with the best key, its row
//                and the count of each output in registers, updated by selects;
//                a strict "better than" keeps the first occurrence.  It writes
//                4 finished records.  Staging, loads and predicates as in
//                k_spell_cols, with the register double buffer (4 rows consumed
//                while the next 4 rows' loads are in flight).  Templated on the
//                dtype and shuffled-or-not (18 kernels).
// k_argext_axes : everything else (another dim, strides, index lists, vector
//                mask tables, 1-D variables): one record per chunk output.
//                Correct, no speed target.  Templated on the dtype (10 kernels).
// k_argext_finalize : the index of n records as int32 and the mask byte.
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // k_rec_segments, k_rec_grid
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode, rec_wave_merge

namespace pyas {

// ---------------------------------------------------------------------------
// the record
// ---------------------------------------------------------------------------
// KIND: the data's class (0 float, 1 signed, 2 unsigned: TT<T>::kind); NEG: argmin.
// Written with | and & on purpose: with || and && the integer classes' walk
// and combine kernels keep the record in a stack object (scratch).
template <int KIND, bool NEG>
struct ArgextMerge {
    // b beats a (both hold an element); the values are read as bits and cast to their class
    static __device__ __forceinline__ bool beats(const pyas_argext &b, const pyas_argext &a) {
        const uint64_t xb = a.value.u, yb = b.value.u;
        // (one index is one element; the bits only make the order total for records of any origin)
        const bool first = (b.index < a.index) | ((b.index == a.index) & (yb < xb));
        if constexpr (KIND == 0) {
            const double x = bits_to<double>(xb), y = bits_to<double>(yb);
            const bool xn = x != x, yn = y != y;
            const bool better = NEG ? y < x : y > x;
            return (xn || yn) ? (yn && (!xn || first)) : (better || (y == x && first));
        } else if constexpr (KIND == 1) {
            const int64_t x = (int64_t)xb, y = (int64_t)yb;
            return (NEG ? y < x : y > x) | ((y == x) & first);
        } else {
            return (NEG ? yb < xb : yb > xb) | ((yb == xb) & first);
        }
    }
    static __device__ __forceinline__ pyas_argext merged(const pyas_argext &a, const pyas_argext &b) {
        const bool tb = (a.n == 0) | ((b.n != 0) & beats(b, a));
        pyas_argext r;
        r.value.u = tb ? b.value.u : a.value.u;
        r.index = tb ? b.index : a.index;
        r.n = a.n + b.n;
        return r;
    }
    static __device__ __forceinline__ pyas_argext shfl_xor(const pyas_argext &p, int m) {
        pyas_argext q;
        q.value.u = pyas::shfl_xor(p.value.u, m);
        q.index = pyas::shfl_xor(p.index, m);
        q.n = pyas::shfl_xor(p.n, m);
        return q;
    }
};

// the key the kernels compare: larger is better (its own inverse)
template <typename T>
__device__ __forceinline__ T ax_key(T x, bool neg) {
    if constexpr (TT<T>::kind == 0) return neg ? -x : x;
    else return neg ? (T)~x : x;
}

// The best of one sequence, position after position in increasing index order.
template <typename T>
struct AxAcc {
    T key;
    int32_t idx, n;
    __device__ __forceinline__ void init() {
        key = (T)0;
        idx = 0;
        n = 0;
    }
    // one position (`on` false: masked or not a position of this sequence, nothing changes)
    __device__ __forceinline__ void add(bool on, T kx, int32_t i) {
        bool better = (n == 0) | (kx > key);
        if constexpr (TT<T>::kind == 0) better = better | ((kx != kx) & (key == key));   // the first NaN
        better = better & on;
        key = better ? kx : key;
        idx = better ? i : idx;
        n += on ? 1 : 0;
    }
    __device__ __forceinline__ pyas_argext finish(bool neg) const {
        const T x = ax_key(key, neg);
        uint64_t bits;   // the value in its class, as pyas_scalar carries it
        if constexpr (TT<T>::kind == 0) bits = bits_to<uint64_t>((double)x);
        else if constexpr (TT<T>::kind == 1) bits = (uint64_t)(int64_t)x;
        else bits = (uint64_t)x;
        pyas_argext p;
        p.value.u = n != 0 ? bits : 0;
        p.index = n != 0 ? idx : 0;
        p.n = n;
        return p;
    }
};

// ---------------------------------------------------------------------------
// k_argext_axes: the per-element walk
// ---------------------------------------------------------------------------
// the index inside the chunk along `dim` of selected position q (no register
// array is indexed by a run-time value)
__device__ __forceinline__ int64_t ax_local(const Sel &s, const int32_t *pool, int dim, int64_t q) {
    int64_t li = 0;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d == dim) li = sel_index(s, pool, d, q);
    return li;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_argext_axes(ArgextArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const uint8_t *base = r.data + r.offsets[c];
    const uint32_t red = 1u << a.dim, keep = ~red & ((1u << r.ndim) - 1u);
    int64_t n_keep, n_red;
    axes_extents(s, r.ndim, red, n_keep, n_red);
    pyas_argext *out = a.out + (a.out_offsets ? a.out_offsets[c] : c);
    const int32_t g0 = a.origin[c];   // the global index of the chunk's local index 0
    // position q of output bo into the accumulator
    auto take = [&](const Decomp &bo, int64_t q, AxAcc<T> &acc) {
        Decomp o = bo;
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, red, q, o);
        const T v = load_elem_rt<T>(base, r.chunk_elems, o.mem, a.shuf, a.bswap);
        const bool um = !all_masked(mk, r.tab, o, v);
        acc.add(um, ax_key(v, a.neg), g0 + (int32_t)ax_local(s, r.pool, a.dim, q));
    };
    if (!a.row) {   // a lane per output, its positions in order
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            Decomp bo{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
            AxAcc<T> acc;
            acc.init();
            for (int64_t q = 0; q < n_red; ++q) take(bo, q, acc);
            out[o] = acc.finish(a.neg);
        }
    } else {        // a wave per output: lane k takes positions k, k + 64, ...; the merge is commutative
        constexpr int kWaves = kBlock / kWave, K = TT<T>::kind;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {   // (wave-uniform)
            Decomp bo{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
            AxAcc<T> acc;
            acc.init();
            for (int64_t q = lane; q < n_red; q += kWave) take(bo, q, acc);
            pyas_argext p = acc.finish(a.neg);
            if (a.neg) rec_wave_merge<pyas_argext, ArgextMerge<K, true>>(p);
            else rec_wave_merge<pyas_argext, ArgextMerge<K, false>>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// k_argext_cols: the dense column walk
// ---------------------------------------------------------------------------
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct AxRows {
    static constexpr int U = 4;
    T v[U][kTrendV];
};

// rows q .. q + U - 1 (those below nq) into y
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void ax_fetch(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                         const int32_t *roff, int q, int nq, AxRows<T> &y) {
    constexpr int U = AxRows<T>::U, V = kTrendV;
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

// nq staged rows (roff: their element offsets; row0: the global index of the
// first) into the lane's 4 accumulators, row after row; `in`: which of the 4
// outputs are selected, vec4: all of them and the chunk's rows are aligned.
// Register double buffer: the next U rows' loads are in flight while these U
// rows are walked.
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void ax_rows(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                        const int32_t *roff, int nq, int32_t row0, const MaskT<T> &mk, bool neg,
                                        AxAcc<T> *acc) {
    constexpr int U = AxRows<T>::U, V = kTrendV;
    AxRows<T> cur, nxt;
    ax_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if (q + U < nq) ax_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q + U, nq, nxt);   // (uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q + u < nq) {   // (uniform)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const T v = cur.v[u][k];
                    const bool um = M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v);
                    acc[k].add(in[k] && um, ax_key(v, neg), row0 + q + u);
                }
            }
        }
        cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void ax_rows_m(int mode, const uint8_t *base, int64_t n, int64_t kmem, bool vec4,
                                          const bool *in, const int32_t *roff, int nq, int32_t row0,
                                          const MaskT<T> &mk, bool neg, AxAcc<T> *acc) {
    if (mode == 0) ax_rows<T, SHUF, BSW, 0>(base, n, kmem, vec4, in, roff, nq, row0, mk, neg, acc);
    else if (mode == kMaskRange) ax_rows<T, SHUF, BSW, kMaskRange>(base, n, kmem, vec4, in, roff, nq, row0, mk, neg, acc);
    else ax_rows<T, SHUF, BSW, kMaskAll>(base, n, kmem, vec4, in, roff, nq, row0, mk, neg, acc);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_argext_cols(ArgextColsArgs a) {
    constexpr int V = kTrendV, ES = sizeof(T);
    const ReduceArgs &r = a.r;
    const int nd = r.ndim, L = nd - 1;
    const int64_t col = (int64_t)blockIdx.x / a.bpc, sb = (int64_t)blockIdx.x % a.bpc;
    // The kept dims' selection is the same in every layer of the column: read
    // it from layer 0 (chunk `col`).
    Sel s0;
    load_sel(s0, r.sel, col, nd, r.shape);
    int64_t KO = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d >= 1 && d < L) KO *= s0.cnt[d];
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
    // (as k_spell_cols: a unit-step box, so a column's first output position
    // along d follows from the first chunk's start)
    int64_t kmem = i0, fidx = 0;
    {
        int64_t rest = col, cs = 1;
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (d < nd && d >= 1) {
                const int64_t nc = a.n_coords[d];
                const int64_t ad = rest % nc;
                rest /= nc;
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
    AxAcc<T> acc[V];
#pragma unroll
    for (int k = 0; k < V; ++k) acc[k].init();
    for (int64_t l = 0; l < a.n_layers; ++l) {
        const int64_t c = l * a.n_cols + col;
        const uint8_t *base = r.data + r.offsets[c];
        // dim 0's selection of this layer
        int64_t rst = 0, R = r.shape[0];
        if (r.sel) {
            const int32_t *p = r.sel + c * PYAS_MAX_DIMS * 3;
            rst = p[0];
            R = p[2];
        }
        const int32_t row_g = a.origin[c] + (int32_t)rst;   // the global index of the layer's first selected row
        const bool vec4 = full && vec_geom && (((uintptr_t)base & (kAlign - 1)) == 0);
        for (int64_t t0 = 0; t0 < R; t0 += kTrendRows) {
            const int nq = (int)(R - t0 < kTrendRows ? R - t0 : kTrendRows);
            __syncthreads();   // the previous pass has been read
            for (int q = threadIdx.x; q < nq; q += kBlock)
                s_roff[q] = (int32_t)((rst + t0 + q) * r.cstride[0]);   // < chunk elements < 2^31
            __syncthreads();
            if (live) {
                const int32_t row0 = row_g + (int32_t)t0;
                if (a.bswap) ax_rows_m<T, SHUF, true>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, row0, mk, a.neg, acc);
                else ax_rows_m<T, SHUF, false>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, row0, mk, a.neg, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (in[k]) a.out[fidx + k * a.ostride[L]] = acc[k].finish(a.neg);
}

// ---------------------------------------------------------------------------
// k_argext_finalize
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_argext_finalize(const pyas_argext *in, int64_t n, int32_t *index,
                                                            uint8_t *masked) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const pyas_argext p = in[i];
    const bool empty = p.n == 0;
    index[i] = empty ? 0 : p.index;
    masked[i] = empty ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_ax_axes_t(const ArgextArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_argext_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_argext_axes(int dtype, const ArgextArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_ax_axes_t, a, grid, st)
}

hipError_t launch_argext_cols(int dtype, const ArgextColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_argext_cols), a, shuf, grid, 0, st)
}

// the data's class of a dtype: 0 float, 1 signed, 2 unsigned
static int ax_kind(int dtype) {
    if (dtype == PYAS_F32 || dtype == PYAS_F64) return 0;
    return (dtype == PYAS_I8 || dtype == PYAS_I16 || dtype == PYAS_I32 || dtype == PYAS_I64) ? 1 : 2;
}

// KN = 2 * class + (argmin ? 1 : 0): the merge as a launcher the combines' checks take
template <int KN>
hipError_t launch_ax_segments(const pyas_argext *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                              pyas_argext *out, hipStream_t st) {
    return launch_rec_segments<pyas_argext, ArgextMerge<KN / 2, (KN & 1) != 0>>(in, index, seg, n_seg, out, st);
}

template <int KN>
hipError_t launch_ax_grid(const pyas_argext *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                          pyas_argext *out, hipStream_t st) {
    return launch_rec_grid<pyas_argext, ArgextMerge<KN / 2, (KN & 1) != 0>>(in, g, n_out, n_layers, out, st);
}

argext_segments_fn launch_argext_segments(int dtype, bool neg) {
    static const argext_segments_fn fn[6] = {launch_ax_segments<0>, launch_ax_segments<1>, launch_ax_segments<2>,
                                             launch_ax_segments<3>, launch_ax_segments<4>, launch_ax_segments<5>};
    return fn[ax_kind(dtype) * 2 + (neg ? 1 : 0)];
}

argext_grid_fn launch_argext_grid(int dtype, bool neg) {
    static const argext_grid_fn fn[6] = {launch_ax_grid<0>, launch_ax_grid<1>, launch_ax_grid<2>,
                                         launch_ax_grid<3>, launch_ax_grid<4>, launch_ax_grid<5>};
    return fn[ax_kind(dtype) * 2 + (neg ? 1 : 0)];
}

hipError_t launch_argext_finalize(const pyas_argext *in, int64_t n, int32_t *index, uint8_t *masked,
                                  hipStream_t st) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_argext_finalize, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, index, masked);
    return hipGetLastError();
}

}  // namespace pyas
