// pyas_rolling.hip — running-window kernels behind Active.rolling
// (pyas_roll_axes, pyas_roll_cols, the two roll combines and
// pyas_roll_finalize of include/pyas.h).
//
// A window is w positions consecutive in the selection along one dim, valid
// when all of them are unmasked; its sum is formed in float64, oldest element
// first (pyas_rolling.hpp).  The record (pyas_roll) keeps the extreme valid
// sum of a sequence piece and the piece's first and last w - 1 elements, so
// that a merge can form the windows across a seam by the same additions.  The
// merge is associative but not commutative, so nothing here merges records
// across lanes: a sequence is walked in order by one lane, and the combines of
// pyas_records.hpp fold the chunks' records sequentially in sequence order.
// Every sum is the same chain of additions on every path, so every path gives
// the same record, byte for byte.
//
// k_roll_cols : the dense path, k_spell_cols (pyas_spell.hip) with another
//               accumulator.  Unit-step box queries with dim 0 the one reduced
//               dim.  A lane owns kTrendV = 4 consecutive outputs along the
//               innermost dim and walks every row of every chunk layer of its
//               column in increasing index order, with the previous w - 1
//               elements of each output in a statically indexed shift register
//               (w is wave-uniform: it only predicates); it writes 4 finished
//               records, the head of each slot by slot while the first w - 1 rows pass.
//               Staging, loads and predicates as in k_spell_cols.  Templated on
//               the dtype and shuffled-or-not (18 kernels).
// k_roll_axes : everything else (another dim, strides, index lists, vector
//               mask tables, 1-D variables): a lane per chunk output, its
//               positions in order.  Correct, no speed target.  Templated on
//               the dtype (10 kernels).
// k_roll_finalize : the sum or the mean of n records as float64 and the mask byte.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pyas_records.hpp"     // k_rec_segments, k_rec_grid
#include "pyas_rolling.hpp"     // RollMerge, RollAcc
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode

namespace pyas {

// The previous elements stay in the variable's own type (half the registers,
// and float64(x) is one instruction) except for the 8-byte integers, whose
// conversion is a sequence of instructions: those are held converted.
template <typename T>
using RollPrev = typename std::conditional<(sizeof(T) == 8), double, T>::type;
template <typename T>
using RollAccT = RollAcc<T, RollPrev<T>>;

// ---------------------------------------------------------------------------
// k_roll_axes: the per-element walk
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_roll_axes(RollArgs a) {
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
    pyas_roll *out = a.out + (a.out_offsets ? a.out_offsets[c] : c);
    const int w = a.window;
    const bool mn = a.which == PYAS_ROLL_MIN;
    // a lane per output, its positions in order
    for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
        Decomp bo{0, {0, 0}};
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
        RollAccT<T> acc;
        acc.init();
        for (int64_t q = 0; q < n_red; ++q) {
            Decomp e = bo;
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, red, q, e);
            const T v = load_elem_rt<T>(base, r.chunk_elems, e.mem, a.shuf, a.bswap);
            const bool um = !all_masked(mk, r.tab, e, v);
            if (acc.len < w - 1) acc.head_slot(out + o, v, um);
            acc.add(v, um, w, mn);
        }
        acc.finish(out + o, w, mn);
    }
}

// ---------------------------------------------------------------------------
// k_roll_cols: the dense column walk
// ---------------------------------------------------------------------------
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct RlRows {
    static constexpr int U = 4;
    T v[U][kTrendV];
};

// rows q .. q + U - 1 (those below nq) into y
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void rl_fetch(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                         const int32_t *roff, int q, int nq, RlRows<T> &y) {
    constexpr int U = RlRows<T>::U, V = kTrendV;
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

// nq staged rows (roff: their element offsets) into the lane's 4 accumulators,
// row after row; `in`: which of the 4 outputs are selected (the accumulator of
// one that is not runs on zeros and is never written), vec4: all of them and
// the chunk's rows are aligned.  Register double buffer: the next U rows' loads
// are in flight while these U rows are walked.
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void rl_rows(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                        const int32_t *roff, int nq, const MaskT<T> &mk, int w, bool mn,
                                        pyas_roll *const *out, RollAccT<T> *acc) {
    constexpr int U = RlRows<T>::U, V = kTrendV;
    RlRows<T> cur, nxt;
    rl_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if (q + U < nq) rl_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q + U, nq, nxt);   // (uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q + u < nq) {   // (uniform)
                const bool head = acc[0].len < w - 1;   // (the same rows for every output of every lane)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const T v = cur.v[u][k];
                    const bool um = M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v);
                    if (head && out[k]) acc[k].head_slot(out[k], v, um);
                    acc[k].add(v, um, w, mn);
                }
            }
        }
        cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void rl_rows_m(int mode, const uint8_t *base, int64_t n, int64_t kmem, bool vec4,
                                          const bool *in, const int32_t *roff, int nq, const MaskT<T> &mk, int w,
                                          bool mn, pyas_roll *const *out, RollAccT<T> *acc) {
    if (mode == 0) rl_rows<T, SHUF, BSW, 0>(base, n, kmem, vec4, in, roff, nq, mk, w, mn, out, acc);
    else if (mode == kMaskRange) rl_rows<T, SHUF, BSW, kMaskRange>(base, n, kmem, vec4, in, roff, nq, mk, w, mn, out, acc);
    else rl_rows<T, SHUF, BSW, kMaskAll>(base, n, kmem, vec4, in, roff, nq, mk, w, mn, out, acc);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_roll_cols(RollColsArgs a) {
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
    // (inlined by hand: past a kernel of this size the inliner leaves a call, and the arguments would go to memory for it)
    [[clang::always_inline]] mk.init(r.mask);
    const int mode = mask_mode(a.masked, r.mask.flags);
    // 4-element loads: every row of the chunk starts at a multiple of 4 elements
    // (and so does every byte plane of a shuffled chunk)
    constexpr int64_t kAlign = (SHUF && ES > 1) ? 4 : (ES * V < 16 ? ES * V : 16);
    const bool vec_geom = (r.shape[L] % V) == 0;
    __shared__ int32_t s_roff[kTrendRows];
    const int w = a.window;
    const bool mn = a.which == PYAS_ROLL_MIN;
    // the records of the lane's outputs (NULL for one that is not selected)
    pyas_roll *out[V];
#pragma unroll
    for (int k = 0; k < V; ++k) out[k] = in[k] ? a.out + fidx + k * a.ostride[L] : nullptr;
    RollAccT<T> acc[V];
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
        const bool vec4 = full && vec_geom && (((uintptr_t)base & (kAlign - 1)) == 0);
        for (int64_t t0 = 0; t0 < R; t0 += kTrendRows) {
            const int nq = (int)(R - t0 < kTrendRows ? R - t0 : kTrendRows);
            __syncthreads();   // the previous pass has been read
            for (int q = threadIdx.x; q < nq; q += kBlock)
                s_roff[q] = (int32_t)((rst + t0 + q) * r.cstride[0]);   // < chunk elements < 2^31
            __syncthreads();
            if (live) {
                if (a.bswap) rl_rows_m<T, SHUF, true>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, w, mn, out, acc);
                else rl_rows_m<T, SHUF, false>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, w, mn, out, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (in[k]) acc[k].finish(out[k], w, mn);
}

// ---------------------------------------------------------------------------
// k_roll_finalize
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_roll_finalize(const pyas_roll *in, int64_t n, int32_t stat, double *value,
                                                          uint8_t *masked) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double best = in[i].best;
    const int32_t nw = in[i].n_windows;
    const int w = in[i].window;
    const bool empty = nw == 0;
    value[i] = empty ? 0.0 : (stat == PYAS_ROLL_MEAN ? best / (double)w : best);
    masked[i] = empty ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_rl_axes_t(const RollArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_roll_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_roll_axes(int dtype, const RollArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_rl_axes_t, a, grid, st)
}

hipError_t launch_roll_cols(int dtype, const RollColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_roll_cols), a, shuf, grid, 0, st)
}

// 144-byte records: 2 in flight (8 of them would not fit the registers)
hipError_t launch_roll_segments(const pyas_roll *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_roll *out, hipStream_t st) {
    return launch_rec_segments<pyas_roll, RollMerge, 2>(in, index, seg, n_seg, out, st);
}

hipError_t launch_roll_grid(const pyas_roll *in, const pyas_grid &g, int64_t n_out, int64_t n_layers, pyas_roll *out,
                            hipStream_t st) {
    return launch_rec_grid<pyas_roll, RollMerge>(in, g, n_out, n_layers, out, st);
}

hipError_t launch_roll_finalize(const pyas_roll *in, int64_t n, int32_t stat, double *value, uint8_t *masked,
                                hipStream_t st) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_roll_finalize, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, stat, value, masked);
    return hipGetLastError();
}

}  // namespace pyas
