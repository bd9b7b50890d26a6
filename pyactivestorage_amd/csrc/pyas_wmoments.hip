// pyas_wmoments.hip — weighted second-moment kernels behind Active.var / std /
// cov / corr with weights= (pyas_wcomoments_axes and the two wcomoments
// combines of include/pyas.h).
//
// One pass over the bytes the unweighted queries read.  The weight of an
// element is the product of one factor per chunk dim, as in pyas_weighted.hip
// (the look-ups of pyas_wvec.hpp); a pair counts when it is selected and
// unmasked on both sides, each side under its own mask.  Per lane, in f64 with
// FMA: n, sw = sum w, sw2 = sum w^2 and the shifted sums s1x = sum w (x - Kx),
// s2x = sum w (x - Kx)^2 and, for two variables, s1y, s2y and
// sxy = sum w (x - Kx)(y - Ky).  The shifts are the lane's first counted
// element of weight > 0 and 0 before it: every earlier term has weight exactly
// 0, so it is exactly 0, or NaN for a NaN or an infinity.  An uncounted value
// or one of weight 0 therefore never becomes the shift, and a counted NaN
// reaches the sums at any weight.  A lane finishes to
//   mean = K + s1/sw,  m2 = s2 - s1^2/sw,  cxy = sxy - s1x s1y/sw
// (sw == 0: mean 0, m2 = s2, cxy = sxy).  Everything above a lane merges
// pyas_wcomoments records with the weighted Chan formula in the fixed order of
// the moments records, so a result is bit-identical from run to run.  Masked
// elements are excluded by select (weight and value both; never multiplied
// by 0).
//
// k_wcom_full : every dim reduced, one workgroup per (chunk, tile).  A whole
//               chunk or a selection that is one contiguous run streams 16-B
//               loads from one or two buffers, register double-buffered, with
//               the factors by digit from LDS (rank <= 3, up to kWLds factors)
//               or from the pool.  Two buffers whose bases are misaligned
//               differently or that differ in shuffle, anything that is not
//               one run, and innermost extents shorter than a vector walk per
//               element.
// k_wcom_axes : partial axes, one record per kept output, the per-element walk
//               with the factor look-ups.  Innermost dim kept: a lane per
//               output; innermost dim reduced: a wave per output.
// k_wcom_full is templated on the dtype, shuffled-or-not and one-or-two
// variables (36 kernels), k_wcom_axes on the dtype and one-or-two variables (20
// kernels: its loads are per element, so each side's shuffle is a run-time
// branch).  Byte order, mask rules and selection kind are run-time branches.
// The file is compiled once per PYAS_WCOM_PART: 1 holds the one-variable
// kernels and the combines, 2 the two-variable kernels.
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // the tile / segment / grid combines
#include "pyas_stat_walk.hpp"   // the tile share, the record merges, load_elem_bsw
#include "pyas_wvec.hpp"        // WVec, VecPos, vec_weights, elem_weight, ws_mask_init, ws_keep

#ifndef PYAS_WCOM_PART
#error "compile with -DPYAS_WCOM_PART=1 (one variable, combines) or 2 (two variables)"
#endif

namespace pyas {

struct WcomMerge {
    // a then b.  Both sides hold weight: the weighted Chan formula.  A side of
    // sw == 0 gives no mean, but its m2s and cxy (each exactly 0, or NaN from a
    // NaN at weight 0) are still added.
    static __device__ __forceinline__ pyas_wcomoments merged(const pyas_wcomoments &a, const pyas_wcomoments &b) {
        const bool both = a.sw > 0.0 && b.sw > 0.0;
        pyas_wcomoments r;
        r.count = a.count + b.count;
        r.sw = a.sw + b.sw;
        r.sw2 = a.sw2 + b.sw2;
        const double dx = both ? b.mean_x - a.mean_x : 0.0, dy = both ? b.mean_y - a.mean_y : 0.0;
        const double f = both ? b.sw / r.sw : 0.0;
        const bool from_b = b.sw > 0.0;   // (not both) the side that has a mean
        r.mean_x = both ? a.mean_x + dx * f : (from_b ? b.mean_x : a.mean_x);
        r.mean_y = both ? a.mean_y + dy * f : (from_b ? b.mean_y : a.mean_y);
        const double m2x = a.m2_x + b.m2_x + dx * dx * a.sw * f;
        const double m2y = a.m2_y + b.m2_y + dy * dy * a.sw * f;
        r.m2_x = m2x < 0.0 ? 0.0 : m2x;   // NaN stays NaN
        r.m2_y = m2y < 0.0 ? 0.0 : m2y;
        r.cxy = a.cxy + b.cxy + dx * dy * a.sw * f;
        return r;
    }
    static __device__ __forceinline__ pyas_wcomoments shfl_xor(const pyas_wcomoments &p, int m) {
        pyas_wcomoments q;
        q.count = pyas::shfl_xor(p.count, m);
        q.sw = pyas::shfl_xor(p.sw, m);
        q.sw2 = pyas::shfl_xor(p.sw2, m);
        q.mean_x = pyas::shfl_xor(p.mean_x, m);
        q.mean_y = pyas::shfl_xor(p.mean_y, m);
        q.m2_x = pyas::shfl_xor(p.m2_x, m);
        q.m2_y = pyas::shfl_xor(p.m2_y, m);
        q.cxy = pyas::shfl_xor(p.cxy, m);
        return q;
    }
};

#if PYAS_WCOM_PART == 1
constexpr bool kTwo = false;
#else
constexpr bool kTwo = true;
#endif

// TWO = false: y is never read (callers pass x again) and its sums stay 0
template <bool TWO>
struct WcAcc {
    double Kx, Ky, sw, sw2, s1x, s2x, s1y, s2y, sxy;
    uint32_t n;
    __device__ __forceinline__ void init() {
        Kx = 0.0; Ky = 0.0; sw = 0.0; sw2 = 0.0; s1x = 0.0; s2x = 0.0; s1y = 0.0; s2y = 0.0; sxy = 0.0; n = 0;
    }
    // weight w (0 for an element that does not count) of the shifted values
    __device__ __forceinline__ void add_d(double w, double dx, double dy) {
        sw += w;
        sw2 = __builtin_fma(w, w, sw2);
        const double wx = w * dx;            // wx dx >= 0: the terms of s2x are non-negative
        s1x += wx;
        s2x = __builtin_fma(wx, dx, s2x);
        if constexpr (TWO) {
            const double wy = w * dy;
            s1y += wy;
            s2y = __builtin_fma(wy, dy, s2y);
            sxy = __builtin_fma(wx, dy, sxy);
        }
    }
    // One element or pair; ok = selected and unmasked (on both sides).  An
    // element that does not count is replaced by weight 0 and value 0 in its own
    // type (one select of a 4-byte value): its terms are 0 (0 - K) = 0 exactly.
    template <typename T>
    __device__ __forceinline__ void add_one(T x, T y, double w, bool ok) {
        const double wv = ok ? w : 0.0;
        const double xs = (double)(ok ? x : (T)0), ys = TWO ? (double)(ok ? y : (T)0) : 0.0;
        const bool first = wv > 0.0 && sw == 0.0;
        Kx = first ? xs : Kx;
        if constexpr (TWO) Ky = first ? ys : Ky;
        add_d(wv, xs - Kx, ys - Ky);
        n += ok ? 1u : 0u;
    }
    // the shifts are set (sw > 0)
    template <typename T>
    __device__ __forceinline__ void add_next(T x, T y, double w, bool ok) {
        const double xs = (double)(ok ? x : (T)0), ys = TWO ? (double)(ok ? y : (T)0) : 0.0;
        add_d(ok ? w : 0.0, xs - Kx, ys - Ky);
        n += ok ? 1u : 0u;
    }
    template <int M, typename T>
    static __device__ __forceinline__ bool pair_ok(T x, T y, const MaskT<T> &mkx, const MaskT<T> &mky) {
        if constexpr (M == 0) return true;
        bool bad = mkx.template masked_m<M>(x);
        if constexpr (TWO) bad |= mky.template masked_m<M>(y);
        return !bad;
    }
    // N elements or pairs; M: mask mode of both sides (0 none, kMaskRange,
    // kMaskAll).  Once every lane that runs this call has its shifts, they are
    // no longer looked for.
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const T *y, const double *w, const MaskT<T> &mkx,
                                          const MaskT<T> &mky) {
        if (__builtin_expect(__ballot(sw == 0.0) != 0, 0)) {
#pragma unroll
            for (int k = 0; k < N; ++k)
                add_one(x[k], y[k], w[k], pair_ok<M>(x[k], y[k], mkx, mky));
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k)
                add_next(x[k], y[k], w[k], pair_ok<M>(x[k], y[k], mkx, mky));
        }
    }
    __device__ __forceinline__ pyas_wcomoments finish() const {
        pyas_wcomoments p;
        const bool has = sw > 0.0;
        const double mux = has ? s1x / sw : 0.0, muy = has ? s1y / sw : 0.0;
        const double m2x = __builtin_fma(-s1x, mux, s2x), m2y = __builtin_fma(-s1y, muy, s2y);
        const double c = __builtin_fma(-s1x, muy, sxy);
        p.count = (int64_t)n;
        p.sw = sw;
        p.sw2 = sw2;
        p.mean_x = has ? Kx + mux : 0.0;
        p.m2_x = m2x < 0.0 ? 0.0 : m2x;   // a rounding residue; NaN stays NaN
        if constexpr (TWO) {
            p.mean_y = has ? Ky + muy : 0.0;
            p.m2_y = m2y < 0.0 ? 0.0 : m2y;
            // not clamped.  A NaN m2 (a counted NaN or +-inf on that side) makes cxy NaN
            p.cxy = (m2x != m2x || m2y != m2y) ? __builtin_nan("") : c;
        } else {
            p.mean_y = 0.0;
            p.m2_y = 0.0;
            p.cxy = 0.0;
        }
        return p;
    }
};

// How the two sides load; the selection and geometry are x's.
struct WcSide {
    const uint8_t *bx, *by;
    bool bsx, bsy, shx, shy;     // shx / shy: only read by the per-element walks
    bool ytabs;                  // y has vector mask tables: its table indices are walked too
};

// RT: some side is byte-swapped (a run-time flag per side); else no branch
template <typename T, bool RT>
__device__ __forceinline__ void wc_unpack(const uint4 &r, T *x, bool bsw) {
    if constexpr (RT) {
        if (bsw) unpack16<T, true>(r, x);
        else unpack16<T, false>(r, x);
    } else {
        unpack16<T, false>(r, x);
    }
}

template <typename T, bool SHUF, bool RT>
__device__ __forceinline__ T wc_load(const uint8_t *base, int64_t n, int64_t i, bool bsw) {
    if constexpr (RT) return load_elem_bsw<T, SHUF>(base, n, i, bsw);
    else return load_elem<T, SHUF, false>(base, n, i);
}

// ---------------------------------------------------------------------------
// contiguous runs: chunk elements [m0, m1) of one or both buffers
// ---------------------------------------------------------------------------
// one element (heads, tails, short runs): a division per dim for its weight
template <typename T, bool SHUF, int M, bool RT, bool WL, int K, bool TWO>
__device__ __forceinline__ void wc_one(const WcSide &cs, int64_t n, int64_t i, WcAcc<TWO> &acc, const MaskT<T> &mkx,
                                       const MaskT<T> &mky, const WVec<WL, K> &wv) {
    const T x = wc_load<T, SHUF, RT>(cs.bx, n, i, cs.bsx);
    T y = x;
    if constexpr (TWO) y = wc_load<T, SHUF, RT>(cs.by, n, i, cs.bsy);
    const double w = elem_weight(wv, i);
    acc.template add_n<1, M>(&x, &y, &w, mkx, mky);
}

// Plain layout.  The vector path of two buffers needs the same head and tail on
// both sides, i.e. bases misaligned alike.
template <typename T, int M, bool RT, bool WL, int K, bool TWO>
__device__ __forceinline__ void wc_run_plain(const WcSide &cs, int64_t m0, int64_t m1, WcAcc<TWO> &acc,
                                             const MaskT<T> &mkx, const MaskT<T> &mky, const WVec<WL, K> &wv) {
    constexpr int ES = sizeof(T);
    constexpr int N = 16 / ES;
    const int tid = threadIdx.x;
    const int64_t b0 = m0 * ES, b1 = m1 * ES;               // byte range in the chunk
    const int64_t mis = (int64_t)((uintptr_t)cs.bx & 15);
    const int64_t a0 = ((b0 + mis + 15) & ~(int64_t)15) - mis;  // first 16-B aligned byte
    const int64_t a1 = ((b1 + mis) & ~(int64_t)15) - mis;
    const bool alike = !TWO || mis == (int64_t)((uintptr_t)cs.by & 15);
    if (!alike || a0 >= a1) {
        for (int64_t i = m0 + tid; i < m1; i += kBlock) wc_one<T, false, M, RT>(cs, 0, i, acc, mkx, mky, wv);
        return;
    }
    const int64_t nhead = (a0 - b0) / ES, ntail = (b1 - a1) / ES;
    if (tid < nhead + ntail)   // fewer than 2 N lanes
        wc_one<T, false, M, RT>(cs, 0, tid < nhead ? m0 + tid : m1 - ntail + (tid - nhead), acc, mkx, mky, wv);
    const uint4 *vx = reinterpret_cast<const uint4 *>(cs.bx + a0);
    const uint4 *vy = reinterpret_cast<const uint4 *>((TWO ? cs.by : cs.bx) + a0);
    const int64_t nvec = (a1 - a0) / 16;
    // this lane's vectors are tid, tid + kBlock, ...: one position, stepped in order
    VecPos<K> pos;
    pos.init(wv, (uint32_t)(a0 / ES + (int64_t)tid * N), (uint32_t)(kBlock * N));
    auto take = [&](const uint4 &rx, const uint4 &ry) {
        T x[N], y[N];
        double w[N];
        wc_unpack<T, RT>(rx, x, cs.bsx);
        if constexpr (TWO) wc_unpack<T, RT>(ry, y, cs.bsy);
        vec_weights<N>(wv, pos, w);
        pos.advance(wv);
        acc.template add_n<N, M>(x, TWO ? y : x, w, mkx, mky);
    };
    constexpr int U = TWO ? 2 : 4;   // per stream: two streams hold the 4 + 4 vectors of one
    constexpr int64_t STEP = (int64_t)U * kBlock;
    const int64_t nsteps = nvec / STEP;
    if (nsteps > 0) {
        uint4 cx[U], nx[U], cy[TWO ? U : 1], ny[TWO ? U : 1];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cx[u] = ldg16(vx + tid + u * kBlock);
            if constexpr (TWO) cy[u] = ldg16(vy + tid + u * kBlock);
        }
        for (int64_t s = 0; s + 1 < nsteps; ++s) {
            // the next step's loads are in flight while this step is reduced
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nx[u] = ldg16(vx + (s + 1) * STEP + tid + u * kBlock);
                if constexpr (TWO) ny[u] = ldg16(vy + (s + 1) * STEP + tid + u * kBlock);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) take(cx[u], cy[TWO ? u : 0]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cx[u] = nx[u];
                if constexpr (TWO) cy[u] = ny[u];
            }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) take(cx[u], cy[TWO ? u : 0]);
    }
    for (int64_t k = nsteps * STEP + tid; k < nvec; k += kBlock) {
        const uint4 rx = ldg16(vx + k);
        uint4 ry = rx;
        if constexpr (TWO) ry = ldg16(vy + k);
        take(rx, ry);
    }
}

// Shuffled layout (both sides), chunk elements [i0, i1) in groups of 16;
// n = elements in the chunk.
template <typename T, int M, bool RT, bool WL, int K, bool TWO>
__device__ __forceinline__ void wc_run_shuffled(const WcSide &cs, int64_t n, int64_t i0, int64_t i1, WcAcc<TWO> &acc,
                                                const MaskT<T> &mkx, const MaskT<T> &mky, const WVec<WL, K> &wv) {
    constexpr int ES = sizeof(T);
    const int tid = threadIdx.x;
    const bool vec_ok = (((uintptr_t)cs.bx & 15) == 0) && (!TWO || ((uintptr_t)cs.by & 15) == 0) && ((n & 15) == 0);
    const int64_t g0 = (i0 + 15) & ~(int64_t)15, g1 = i1 & ~(int64_t)15;
    if (!vec_ok || g0 >= g1) {
        for (int64_t i = i0 + tid; i < i1; i += kBlock) wc_one<T, true, M, RT>(cs, n, i, acc, mkx, mky, wv);
        return;
    }
    if (tid < (g0 - i0) + (i1 - g1))   // fewer than 32 lanes
        wc_one<T, true, M, RT>(cs, n, tid < g0 - i0 ? i0 + tid : g1 + (tid - (g0 - i0)), acc, mkx, mky, wv);
    const int64_t ng = (g1 - g0) / 16;
    VecPos<K> pos;
    pos.init(wv, (uint32_t)(g0 + (int64_t)tid * 16), (uint32_t)(kBlock * 16));
    auto group = [&](const uint8_t *base, int64_t i, bool bsw, T *x) {
        uint4 pl[ES];
#pragma unroll
        for (int b = 0; b < ES; ++b) pl[b] = ldg16(reinterpret_cast<const uint4 *>(base + (int64_t)b * n + i));
        if constexpr (RT) {
            if (bsw) unshuffle16<T, true>(pl, x);
            else unshuffle16<T, false>(pl, x);
        } else {
            unshuffle16<T, false>(pl, x);
        }
    };
    for (int64_t g = tid; g < ng; g += kBlock) {
        const int64_t i = g0 + g * 16;
        T x[16], y[TWO ? 16 : 1];
        double w[16];
        group(cs.bx, i, cs.bsx, x);
        if constexpr (TWO) group(cs.by, i, cs.bsy, y);
        vec_weights<16>(wv, pos, w);
        pos.advance(wv);
        acc.template add_n<16, M>(x, TWO ? y : x, w, mkx, mky);
    }
}

template <typename T, bool SHUF, bool RT, bool WL, int K, bool TWO>
__device__ __forceinline__ void wc_run(int mode, const WcSide &cs, int64_t n, int64_t i0, int64_t i1, WcAcc<TWO> &acc,
                                       const MaskT<T> &mkx, const MaskT<T> &mky, const WVec<WL, K> &wv) {
    if constexpr (!WL) {   // beyond the LDS path: one instantiation, which evaluates every mask rule at run time
        if constexpr (SHUF && sizeof(T) > 1) wc_run_shuffled<T, kMaskAll, RT>(cs, n, i0, i1, acc, mkx, mky, wv);
        else wc_run_plain<T, kMaskAll, RT>(cs, i0, i1, acc, mkx, mky, wv);
    } else if constexpr (SHUF && sizeof(T) > 1) {
        if (mode == 0) wc_run_shuffled<T, 0, RT>(cs, n, i0, i1, acc, mkx, mky, wv);
        else if (mode == kMaskRange) wc_run_shuffled<T, kMaskRange, RT>(cs, n, i0, i1, acc, mkx, mky, wv);
        else wc_run_shuffled<T, kMaskAll, RT>(cs, n, i0, i1, acc, mkx, mky, wv);
    } else {
        if (mode == 0) wc_run_plain<T, 0, RT>(cs, i0, i1, acc, mkx, mky, wv);
        else if (mode == kMaskRange) wc_run_plain<T, kMaskRange, RT>(cs, i0, i1, acc, mkx, mky, wv);
        else wc_run_plain<T, kMaskAll, RT>(cs, i0, i1, acc, mkx, mky, wv);
    }
}

// ---------------------------------------------------------------------------
// per-element walk: factors by dim, read from the pool
// ---------------------------------------------------------------------------
// Positions q0, q0 + stride, ... < n_pos over the dims in `dmask` (rc: the
// radix counter at q0).  Dims outside dmask sit at chunk index kli[d] (already
// part of box / boy, the kept dims' part for x's and y's tables); org: the
// chunk's row of origin.
template <typename T, bool TWO>
__device__ __forceinline__ void wc_walk(const ReduceArgs &r, const MaskTab &ty, const WcSide &cs, const Sel &s,
                                        uint32_t dmask, const Decomp &box, const Decomp &boy, const int32_t *kli,
                                        const double *wpool, const int32_t *org, RadixCounter &rc, int64_t q0,
                                        int64_t n_pos, int64_t stride, const MaskT<T> &mkx, const MaskT<T> &mky,
                                        WcAcc<TWO> &acc) {
    auto locate = [&](Decomp &ox, Decomp &oy, double &w) {
        w = 1.0;
#pragma unroll
        for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
            if (d < r.ndim) {
                int64_t li = kli[d];
                if ((dmask >> d) & 1u) {
                    li = sel_index(s, r.pool, d, rc.idx[d]);
                    ox.mem += li * r.cstride[d];
                    ox.v[0] += (int64_t)rc.idx[d] * r.tab.stride[0][d];
                    ox.v[1] += (int64_t)rc.idx[d] * r.tab.stride[1][d];
                    if (TWO && cs.ytabs) {
                        oy.v[0] += (int64_t)rc.idx[d] * ty.stride[0][d];
                        oy.v[1] += (int64_t)rc.idx[d] * ty.stride[1][d];
                    }
                }
                w *= wpool[org[d] + li];
            }
        }
    };
    auto counted = [&](const Decomp &ox, const Decomp &oy, T x, T y) {
        bool bad = all_masked(mkx, r.tab, ox, x);
        if constexpr (TWO) bad |= all_masked(mky, ty, oy, y);
        return !bad;
    };
    const bool shx = cs.shx && sizeof(T) > 1, shy = cs.shy && sizeof(T) > 1;
    constexpr int U = TWO ? 2 : 4;   // 4 loads in flight
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp ox[U], oy[U];
        double w[U];
        T x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ox[u] = box;
            oy[u] = boy;
            locate(ox[u], oy[u], w[u]);
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = load_elem_rt<T>(cs.bx, r.chunk_elems, ox[u].mem, shx, cs.bsx);
            y[u] = x[u];
            if constexpr (TWO) y[u] = load_elem_rt<T>(cs.by, r.chunk_elems, ox[u].mem, shy, cs.bsy);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc.add_one(x[u], y[u], w[u], counted(ox[u], oy[u], x[u], y[u]));
    }
    for (; q < n_pos; q += stride) {
        Decomp ox = box, oy = boy;
        double w;
        locate(ox, oy, w);
        rc.advance();
        const T x = load_elem_rt<T>(cs.bx, r.chunk_elems, ox.mem, shx, cs.bsx);
        T y = x;
        if constexpr (TWO) y = load_elem_rt<T>(cs.by, r.chunk_elems, ox.mem, shy, cs.bsy);
        acc.add_one(x, y, w, counted(ox, oy, x, y));
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF, bool TWO>
__global__ __launch_bounds__(kBlock) void k_wcom_full(WcomArgs a) {
    const ReduceArgs &r = a.x;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, t = (int64_t)blockIdx.x % a.bpc;
    const int32_t *org = a.worigin + c * PYAS_MAX_DIMS;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mkx, mky;
    ws_mask_init(mkx, a.x.mask);
    if constexpr (TWO) ws_mask_init(mky, a.y.mask);
    else mky = mkx;
    const bool ytabs = TWO && (a.y.tab.on[0] || a.y.tab.on[1]);
    const WcSide cs{a.x.data + a.x.offsets[c], TWO ? a.y.data + a.y.offsets[c] : nullptr,
                    a.bswap_x, a.bswap_y, a.shuf_x, a.shuf_y, ytabs};
    // One contiguous run?  From the innermost dim: whole dims, then one
    // unit-step range, then single indices.  (Two sides that differ in
    // shuffle have no common vector layout.)
    constexpr int NV = (SHUF && sizeof(T) > 1) ? 16 : 16 / (int)sizeof(T);   // elements per vector
    int64_t total = 1, m0 = 0, ext = 0;
    bool contig = !(r.tab.on[0] || r.tab.on[1] || ytabs) && !(TWO && a.shuf_x != a.shuf_y), inner_full = true;
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
    // one mode for both sides: the wider of the two (a rule a side does not
    // have compares against its neutral thresholds)
    const int mx = mask_mode(a.masked_x, a.x.mask.flags), my = TWO ? mask_mode(a.masked_y, a.y.mask.flags) : 0;
    const int mode = (mx == kMaskAll || my == kMaskAll) ? kMaskAll : (mx | my);
    const bool bsw = a.bswap_x || (TWO && a.bswap_y);
    __shared__ double s_wt[kWLds];
    WcAcc<TWO> acc;
    acc.init();
    if (contig && r.ndim <= 3 && ext <= kWLds) {       // (uniform)
        WVec<true, 3> wv;
        wvec_setup(wv, r, a.wpool, org, s_wt);
        __syncthreads();
        if (e0 < e1) {
            if (bsw) wc_run<T, SHUF, true>(mode, cs, r.chunk_elems, m0 + e0, m0 + e1, acc, mkx, mky, wv);
            else wc_run<T, SHUF, false>(mode, cs, r.chunk_elems, m0 + e0, m0 + e1, acc, mkx, mky, wv);
        }
    } else if (contig) {
        WVec<false, PYAS_MAX_DIMS> wv;
        wvec_setup(wv, r, a.wpool, org, s_wt);
        if (e0 < e1) {
            if (bsw) wc_run<T, SHUF, true>(mode, cs, r.chunk_elems, m0 + e0, m0 + e1, acc, mkx, mky, wv);
            else wc_run<T, SHUF, false>(mode, cs, r.chunk_elems, m0 + e0, m0 + e1, acc, mkx, mky, wv);
        }
    } else if (e0 + threadIdx.x < e1) {
        const uint32_t all = (1u << r.ndim) - 1u;
        RadixCounter rc;
        rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
        const Decomp zero{0, {0, 0}};
        const int32_t kli[PYAS_MAX_DIMS] = {0, 0, 0, 0, 0, 0, 0, 0};
        wc_walk<T, TWO>(r, a.y.tab, cs, s, all, zero, zero, kli, a.wpool, org, rc, e0 + threadIdx.x, e1, kBlock, mkx,
                        mky, acc);
    }
    rec_store_full<WcomMerge>(acc, a, c);
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T, bool TWO>
__global__ __launch_bounds__(kBlock) void k_wcom_axes(WcomArgs a) {
    const ReduceArgs &r = a.x;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const int32_t *org = a.worigin + c * PYAS_MAX_DIMS;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mkx, mky;
    ws_mask_init(mkx, a.x.mask);
    if constexpr (TWO) ws_mask_init(mky, a.y.mask);
    else mky = mkx;
    const bool ytabs = TWO && (a.y.tab.on[0] || a.y.tab.on[1]);
    const WcSide cs{a.x.data + a.x.offsets[c], TWO ? a.y.data + a.y.offsets[c] : nullptr,
                    a.bswap_x, a.bswap_y, a.shuf_x, a.shuf_y, ytabs};
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep, n_red;
    axes_extents(s, r.ndim, red, n_keep, n_red);
    pyas_wcomoments *out = a.out + a.out_offsets[c];
    // output o's kept part: x's memory, tables and chunk indices; y's tables
    auto kept_part = [&](int64_t o, Decomp &box, Decomp &boy, int32_t *kli) {
        box = Decomp{0, {0, 0}};
        boy = Decomp{0, {0, 0}};
        ws_keep(r, s, keep, o, box, kli);
        if (ytabs) decompose(s, r.pool, r.cstride, a.y.tab, r.ndim, keep, o, boy);
        boy.mem = 0;
    };
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            WcAcc<TWO> acc;
            acc.init();
            if (n_red > 0) {
                Decomp box, boy;
                int32_t kli[PYAS_MAX_DIMS];
                kept_part(o, box, boy, kli);
                RadixCounter rc;
                rc.init(s, r.ndim, red, 0, 1);
                wc_walk<T, TWO>(r, a.y.tab, cs, s, red, box, boy, kli, a.wpool, org, rc, 0, n_red, 1, mkx, mky, acc);
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            WcAcc<TWO> acc;
            acc.init();
            if (lane < n_red) {
                Decomp box, boy;
                int32_t kli[PYAS_MAX_DIMS];
                kept_part(o, box, boy, kli);
                RadixCounter rc;
                rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                wc_walk<T, TWO>(r, a.y.tab, cs, s, red, box, boy, kli, a.wpool, org, rc, lane, n_red, kWave, mkx, mky,
                                acc);
            }
            pyas_wcomoments p = acc.finish();
            rec_wave_merge<pyas_wcomoments, WcomMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// launchers (the two templates are static: each part has its own, with its kTwo)
// ---------------------------------------------------------------------------
template <typename T>
static hipError_t launch_wcom_full_t(const WcomArgs &a, int64_t grid, hipStream_t st) {
    const dim3 g((unsigned)grid), b(kBlock);
    // both sides shuffled: the byte-plane runs; sides that differ walk per element
    if constexpr (sizeof(T) > 1) {
        if (a.shuf_x && (!kTwo || a.shuf_y)) {
            hipLaunchKernelGGL((k_wcom_full<T, true, kTwo>), g, b, 0, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((k_wcom_full<T, false, kTwo>), g, b, 0, st, a);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_wcom_axes_t(const WcomArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_wcom_axes<T, kTwo>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

#if PYAS_WCOM_PART == 1
hipError_t launch_wcom1_full(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_wcom_full_t, a, grid, st)
}

hipError_t launch_wcom1_axes(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_wcom_axes_t, a, grid, st)
}

hipError_t launch_wcom_tiles(const pyas_wcomoments *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                             pyas_wcomoments *out, hipStream_t st) {
    return launch_rec_tiles<pyas_wcomoments, WcomMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

// 64-byte records: 4 in flight
hipError_t launch_wcom_segments(const pyas_wcomoments *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_wcomoments *out, hipStream_t st) {
    return launch_rec_segments<pyas_wcomoments, WcomMerge, 4>(in, index, seg, n_seg, out, st);
}

hipError_t launch_wcom_grid(const pyas_wcomoments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                            pyas_wcomoments *out, hipStream_t st) {
    return launch_rec_grid<pyas_wcomoments, WcomMerge>(in, g, n_out, n_layers, out, st);
}
#else
hipError_t launch_wcom2_full(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_wcom_full_t, a, grid, st)
}

hipError_t launch_wcom2_axes(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_wcom_axes_t, a, grid, st)
}
#endif

}  // namespace pyas
