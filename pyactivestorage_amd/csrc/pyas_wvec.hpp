// pyas_wvec.hpp — the weight of a chunk element as a product of one factor per
// dim, looked up by digit: shared by pyas_weighted.hip (weighted sums) and
// pyas_wmoments.hip (weighted second moments).  The factors of a chunk come
// from LDS (staged once per workgroup, up to kWLds doubles) or from the pool in
// global memory; a contiguous run carries the position of a lane's next vector
// as one digit per dim, so a step is a carry-propagating add, not a division.
#pragma once

#include <hip/hip_runtime.h>

#include "pyas_kernels.hpp"

namespace pyas {

// MaskT<T>::init, always inline: as a call it takes the kernel's arguments by
// address, which puts them (and the full kernel) on the stack.
template <typename T>
__device__ __forceinline__ void ws_mask_init(MaskT<T> &mk, const pyas_mask &m) {
    const T big = TT<T>::highest(), small = TT<T>::lowest();
    const bool e0 = m.flags & PYAS_MASK_EQ0, e1 = m.flags & PYAS_MASK_EQ1;
    mk.lo0 = e0 ? TT<T>::from(m.eq_lo[0]) : big;
    mk.hi0 = e0 ? TT<T>::from(m.eq_hi[0]) : small;
    mk.lo1 = e1 ? TT<T>::from(m.eq_lo[1]) : big;
    mk.hi1 = e1 ? TT<T>::from(m.eq_hi[1]) : small;
    mk.gt = (m.flags & PYAS_MASK_GT) ? TT<T>::from(m.gt) : big;
    mk.lt = (m.flags & PYAS_MASK_LT) ? TT<T>::from(m.lt) : small;
}

// ---------------------------------------------------------------------------
// contiguous runs: factors by digit.  The chunk's dims are right-aligned on K
// digits (digit j is dim j - lo; digits below lo are padding of extent 1).
// ---------------------------------------------------------------------------
constexpr int kWLds = 2048;   // factors of one chunk kept in LDS (f64, 16 KiB)

template <bool WL, int K>
struct WVec {
    const double *tab;     // WL: the chunk's factors in LDS; else the pool
    int32_t off[K];        // start of digit j's factors in tab
    uint32_t cnt[K];       // extent of digit j
    int lo;
    __device__ __forceinline__ double at(int j, uint32_t i) const { return tab[off[j] + (int32_t)i]; }
};

// (WL: every thread of the workgroup calls this, then __syncthreads())
template <bool WL, int K>
__device__ __forceinline__ void wvec_setup(WVec<WL, K> &v, const ReduceArgs &r, const double *pool,
                                           const int32_t *org, double *lds) {
    v.lo = K - r.ndim;
    v.tab = WL ? lds : pool;
    int32_t pos = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        v.cnt[j] = 1;
        v.off[j] = 0;
#pragma unroll
        for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
            if (d < K && d < r.ndim && d == j - v.lo) {
                const int32_t n = (int32_t)r.shape[d];
                const int32_t o = org[d];
                v.cnt[j] = (uint32_t)n;
                if (WL) {
                    for (int32_t i = threadIdx.x; i < n; i += kBlock) lds[pos + i] = pool[o + i];
                    v.off[j] = pos;
                    pos += n;
                } else {
                    v.off[j] = o;
                }
            }
        }
    }
}

// Position of a lane's next vector in the chunk, a digit per dim; divisions
// happen once per run, every step is then a carry-propagating add.
template <int K>
struct VecPos {
    uint32_t idx[K], inc[K];
    template <bool WL>
    __device__ __forceinline__ void init(const WVec<WL, K> &v, uint32_t start, uint32_t stride) {
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            const uint32_t c = v.cnt[j];
            idx[j] = start % c;
            start /= c;
            inc[j] = stride % c;
            stride /= c;
        }
    }
    template <bool WL>
    __device__ __forceinline__ void advance(const WVec<WL, K> &v) {
        uint32_t carry = 0;
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            const uint32_t x = idx[j] + inc[j] + carry;
            carry = x >= v.cnt[j] ? 1u : 0u;
            idx[j] = carry ? x - v.cnt[j] : x;
        }
    }
};

// The weights of the N consecutive chunk elements that start at p; N is at most
// the innermost extent (the caller's condition), so they span at most two rows.
template <int N, bool WL, int K>
__device__ __forceinline__ void vec_weights(const WVec<WL, K> &v, const VecPos<K> &p, double *w) {
    const uint32_t col = p.idx[K - 1], len = v.cnt[K - 1];
    double outer = 1.0;
#pragma unroll
    for (int j = 0; j < K - 1; ++j)
        if (j >= v.lo) outer *= v.at(j, p.idx[j]);
    if (N == 1 || col + N <= len) {   // inside one innermost row
#pragma unroll
        for (int k = 0; k < N; ++k) w[k] = outer * v.at(K - 1, col + k);
    } else {                          // the vector straddles into the next row
        double next = 1.0;
        uint32_t carry = 1;
        uint32_t t[K - 1];
#pragma unroll
        for (int j = K - 2; j >= 0; --j) {
            const uint32_t y = p.idx[j] + carry;
            carry = y >= v.cnt[j] ? 1u : 0u;
            t[j] = carry ? 0u : y;
        }
#pragma unroll
        for (int j = 0; j < K - 1; ++j)
            if (j >= v.lo) next *= v.at(j, t[j]);
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const bool wrap = col + k >= len;
            w[k] = (wrap ? next : outer) * v.at(K - 1, wrap ? col + k - len : col + k);
        }
    }
}

// The weight of chunk element i (divisions: heads, tails and short runs only).
template <bool WL, int K>
__device__ __forceinline__ double elem_weight(const WVec<WL, K> &v, int64_t i) {
    VecPos<K> p;
    p.init(v, (uint32_t)i, 0u);
    double w;
    vec_weights<1>(v, p, &w);
    return w;
}

// Output o's kept coordinates (partial axes): chunk memory, table indices and
// chunk index per kept dim.
__device__ __forceinline__ void ws_keep(const ReduceArgs &r, const Sel &s, uint32_t keep, int64_t e, Decomp &o,
                                        int32_t *kli) {
#pragma unroll
    for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
        kli[d] = 0;
        if (d < r.ndim && ((keep >> d) & 1u)) {
            const int64_t cd = s.cnt[d];
            const int64_t q = e / cd, k = e - q * cd;
            e = q;
            const int64_t li = sel_index(s, r.pool, d, k);
            kli[d] = (int32_t)li;
            o.mem += li * r.cstride[d];
            o.v[0] += k * r.tab.stride[0][d];
            o.v[1] += k * r.tab.stride[1][d];
        }
    }
}

}  // namespace pyas
