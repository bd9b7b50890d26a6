// pyas_spell.hip — spell kernels behind Active.spell (pyas_spell_axes,
// pyas_spell_cols, the two spell combines and pyas_spell_finalize of
// include/pyas.h).
//
// A position is true when its element is unmasked and float64(x) op threshold
// holds; the record (pyas_spell) describes the runs of true positions of a
// sequence.  Its merge is associative but not commutative, so nothing here
// merges records across lanes: a sequence is walked in order by one lane
// (k_spell_cols, k_spell_axes' column layout) or 64 positions at a time by one
// wave through ballots (k_spell_axes' row layout), and the combines of
// pyas_records.hpp fold the chunks' records sequentially in sequence order.
// All arithmetic is integer, so every path gives the same record.
//
// k_spell_cols : the dense path, k_trend_cols (pyas_trend.hip) without the
//                coordinate.  Unit-step box queries with dim 0 the one reduced
//                dim.  A lane owns kTrendV = 4 consecutive outputs along the
//                innermost dim and walks every row of every chunk layer of its
//                column in increasing index order, with the current run, the
//                head and the counts of each output in integer registers; it
//                writes 4 finished records.  Staging, loads and predicates as
//                in k_trend_cols; the accumulator is small, so every type
//                keeps the register double buffer (4 rows consumed while the
//                next 4 rows' loads are in flight).  Templated on the dtype and
//                shuffled-or-not (18 kernels).
// k_spell_axes : everything else (another dim, strides, index lists, vector
//                mask tables, 1-D variables): one record per chunk output.
//                Correct, no speed target.  Templated on the dtype (10 kernels).
// k_spell_finalize : one stat of n records as int32 and the mask byte.
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // k_rec_segments, k_rec_grid
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode

namespace pyas {

// ---------------------------------------------------------------------------
// the record
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t sp_max(int32_t a, int32_t b) { return a > b ? a : b; }

struct SpellMerge {
    // a's positions, then b's.  (No shfl_xor: lane records are never merged.)
    static __device__ __forceinline__ pyas_spell merged(const pyas_spell &a, const pyas_spell &b) {
        const int32_t L = sp_max(a.min_length, b.min_length);
        const bool a_all = a.head == a.len, b_all = b.head == b.len;
        const int32_t j = a.tail + b.head;
        const bool joined = !a_all && !b_all && j >= L;   // the run across the seam is interior
        pyas_spell r;
        r.n = a.n + b.n;
        r.n_true = a.n_true + b.n_true;
        r.len = a.len + b.len;
        r.head = a_all ? a.len + b.head : a.head;
        r.tail = b_all ? b.len + a.tail : b.tail;
        r.best = sp_max(sp_max(a.best, b.best), j);
        r.days = a.days + b.days + (joined ? j : 0);
        r.events = a.events + b.events + (joined ? 1 : 0);
        r.min_length = L;
        r.reserved = 0;
        return r;
    }
};

// float64(x) op threshold; a NaN compares false
template <typename T>
__device__ __forceinline__ bool sp_true(const SpellTest &t, T v) {
    const double x = (double)v;
    const double xs = t.neg ? -x : x;
    return (xs > t.threshold) | (t.incl & (xs == t.threshold));
}

// The runs of one sequence, position after position.
struct SpAcc {
    int32_t cur, head, best, days, events, n, n_true, len;
    bool broken;   // a false position has been seen: the head is fixed
    __device__ __forceinline__ void init() {
        cur = 0; head = 0; best = 0; days = 0; events = 0; n = 0; n_true = 0; len = 0;
        broken = false;
    }
    // one position (`on` false: not a position of this sequence, nothing changes)
    __device__ __forceinline__ void add(bool on, bool is_true, bool unmasked, int32_t L) {
        const bool close = on && !is_true;
        const bool interior = close && broken && cur >= L;   // the run that ends here touches neither end
        head = (close && !broken) ? cur : head;
        days += interior ? cur : 0;
        events += interior ? 1 : 0;
        broken = broken || close;
        cur = close ? 0 : cur + ((on && is_true) ? 1 : 0);
        best = sp_max(best, cur);
        n += (on && unmasked) ? 1 : 0;
        n_true += (on && is_true) ? 1 : 0;
        len += on ? 1 : 0;
    }
    __device__ __forceinline__ pyas_spell finish(int32_t L) const {
        pyas_spell p;
        p.n = n;
        p.n_true = n_true;
        p.len = len;
        p.head = broken ? head : len;
        p.tail = cur;
        p.best = best;
        p.days = days;
        p.events = events;
        p.min_length = L;
        p.reserved = 0;
        return p;
    }
};

// ---------------------------------------------------------------------------
// k_spell_axes: the per-element walk
// ---------------------------------------------------------------------------
// 64 consecutive positions as bits (bit i: position i; nv of them exist):
// tw the true ones, uw the unmasked ones.  Wave-uniform.
__device__ __forceinline__ pyas_spell sp_word(uint64_t tw, uint64_t uw, int nv, int32_t L) {
    pyas_spell p;
    p.n = __builtin_popcountll(uw);
    p.n_true = __builtin_popcountll(tw);
    p.len = nv;
    p.min_length = L;
    p.reserved = 0;
    p.days = 0;
    p.events = 0;
    const uint64_t lo = ~tw;                        // trailing ones of tw
    const int head = lo ? __builtin_ctzll(lo) : 64;
    if (head >= nv) {                               // every position is true
        p.head = nv;
        p.tail = nv;
        p.best = nv;
        return p;
    }
    const uint64_t hi = ~(tw << (64 - nv));         // leading ones of the nv positions (1 <= nv <= 64)
    const int tail = __builtin_clzll(hi);           // hi != 0: position head is false
    p.head = head;
    p.tail = tail;
    int best = 0;
    for (uint64_t m = tw; m; m &= m << 1) ++best;
    p.best = best;
    // the interior runs: those left once the head and the tail run are cleared (head, tail <= 63)
    const uint64_t tmask = tail ? ((uint64_t(1) << tail) - 1u) << (nv - tail) : 0;
    uint64_t x = tw & ~((uint64_t(1) << head) - 1u) & ~tmask;
    while (x) {
        const int s = __builtin_ctzll(x);
        const int r = __builtin_ctzll(~(x >> s));   // <= 62: an interior run has a false position on both sides
        if (r >= L) {
            p.days += r;
            p.events += 1;
        }
        x &= ~(((uint64_t(1) << r) - 1u) << s);
    }
    return p;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_spell_axes(SpellArgs a) {
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
    pyas_spell *out = a.out + (a.out_offsets ? a.out_offsets[c] : c);
    const int32_t L = a.t.min_length;
    // position q of output bo: the element and whether it is unmasked
    auto element = [&](const Decomp &bo, int64_t q, bool &unmasked) {
        Decomp o = bo;
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, red, q, o);
        const T v = load_elem_rt<T>(base, r.chunk_elems, o.mem, a.shuf, a.bswap);
        unmasked = !all_masked(mk, r.tab, o, v);
        return v;
    };
    if (!a.row) {   // a lane per output, its positions in order
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            Decomp bo{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
            SpAcc acc;
            acc.init();
            for (int64_t q = 0; q < n_red; ++q) {
                bool um;
                const T v = element(bo, q, um);
                acc.add(true, um && sp_true(a.t, v), um, L);
            }
            out[o] = acc.finish(L);
        }
    } else {        // a wave per output, 64 positions per step (wave-uniform trip counts)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            Decomp bo{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
            pyas_spell p{};
            p.min_length = L;
            for (int64_t q0 = 0; q0 < n_red; q0 += kWave) {
                const int64_t q = q0 + lane;
                bool um = false, tr = false;
                if (q < n_red) {
                    const T v = element(bo, q, um);
                    tr = um && sp_true(a.t, v);
                }
                const uint64_t tw = __ballot(tr), uw = __ballot(um);
                const int nv = (int)(n_red - q0 < kWave ? n_red - q0 : kWave);
                p = SpellMerge::merged(p, sp_word(tw, uw, nv, L));
            }
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// k_spell_cols: the dense column walk
// ---------------------------------------------------------------------------
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct SpRows {
    static constexpr int U = 4;
    T v[U][kTrendV];
};

// rows q .. q + U - 1 (those below nq) into y
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void sp_fetch(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                         const int32_t *roff, int q, int nq, SpRows<T> &y) {
    constexpr int U = SpRows<T>::U, V = kTrendV;
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
// row after row; `in`: which of the 4 outputs are selected, vec4: all of them
// and the chunk's rows are aligned.  Register double buffer: the next U rows'
// loads are in flight while these U rows are walked.
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void sp_rows(const uint8_t *base, int64_t n, int64_t kmem, bool vec4, const bool *in,
                                        const int32_t *roff, int nq, const MaskT<T> &mk, const SpellTest &t,
                                        SpAcc *acc) {
    constexpr int U = SpRows<T>::U, V = kTrendV;
    SpRows<T> cur, nxt;
    sp_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if (q + U < nq) sp_fetch<T, SHUF, BSW>(base, n, kmem, vec4, in, roff, q + U, nq, nxt);   // (uniform)
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q + u < nq) {   // (uniform)
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const T v = cur.v[u][k];
                    const bool um = M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v);
                    acc[k].add(in[k], um && sp_true(t, v), um, t.min_length);
                }
            }
        }
        cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void sp_rows_m(int mode, const uint8_t *base, int64_t n, int64_t kmem, bool vec4,
                                          const bool *in, const int32_t *roff, int nq, const MaskT<T> &mk,
                                          const SpellTest &t, SpAcc *acc) {
    if (mode == 0) sp_rows<T, SHUF, BSW, 0>(base, n, kmem, vec4, in, roff, nq, mk, t, acc);
    else if (mode == kMaskRange) sp_rows<T, SHUF, BSW, kMaskRange>(base, n, kmem, vec4, in, roff, nq, mk, t, acc);
    else sp_rows<T, SHUF, BSW, kMaskAll>(base, n, kmem, vec4, in, roff, nq, mk, t, acc);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_spell_cols(SpellColsArgs a) {
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
    // (as k_trend_cols: a unit-step box, so a column's first output position
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
    SpAcc acc[V];
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
                if (a.bswap) sp_rows_m<T, SHUF, true>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, a.t, acc);
                else sp_rows_m<T, SHUF, false>(mode, base, r.chunk_elems, kmem, vec4, in, s_roff, nq, mk, a.t, acc);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < V; ++k)
        if (in[k]) a.out[fidx + k * a.ostride[L]] = acc[k].finish(a.t.min_length);
}

// ---------------------------------------------------------------------------
// k_spell_finalize
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_spell_finalize(const pyas_spell *in, int64_t n, int32_t stat,
                                                           int32_t *value, uint8_t *masked) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const pyas_spell p = in[i];
    const int32_t L = p.min_length;
    const bool h = p.head >= L && p.head > 0, t = p.head != p.len && p.tail >= L && p.tail > 0;
    const int32_t v = stat == PYAS_SPELL_LONGEST ? p.best
                      : stat == PYAS_SPELL_DAYS ? p.days + (h ? p.head : 0) + (t ? p.tail : 0)
                                                : p.events + (h ? 1 : 0) + (t ? 1 : 0);
    const bool empty = p.n == 0;
    value[i] = empty ? 0 : v;
    masked[i] = empty ? 1 : 0;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_sp_axes_t(const SpellArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_spell_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_spell_axes(int dtype, const SpellArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_sp_axes_t, a, grid, st)
}

hipError_t launch_spell_cols(int dtype, const SpellColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_spell_cols), a, shuf, grid, 0, st)
}

hipError_t launch_spell_segments(const pyas_spell *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                 pyas_spell *out, hipStream_t st) {
    return launch_rec_segments<pyas_spell, SpellMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_spell_grid(const pyas_spell *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                             pyas_spell *out, hipStream_t st) {
    return launch_rec_grid<pyas_spell, SpellMerge>(in, g, n_out, n_layers, out, st);
}

hipError_t launch_spell_finalize(const pyas_spell *in, int64_t n, int32_t stat, int32_t *value, uint8_t *masked,
                                 hipStream_t st) {
    const int64_t nb = (n + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(k_spell_finalize, dim3((unsigned)nb), dim3(kBlock), 0, st, in, n, stat, value, masked);
    return hipGetLastError();
}

}  // namespace pyas
