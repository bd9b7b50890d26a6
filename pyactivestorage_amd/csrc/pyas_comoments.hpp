// pyas_comoments.hpp — the co-moment record's lane accumulator and merge,
// shared by pyas_comoments.hip (two stored variables) and pyas_trend.hip (one
// variable against a coordinate).  See pyas_comoments.hip for the numerics.
#pragma once

#include "pyas_device.hpp"

namespace pyas {

struct ComomMerge {
    // a then b; the means and m2s exactly as MomMerge::merged (pyas_moments.hpp)
    static __device__ __forceinline__ pyas_comoments merged(const pyas_comoments &a, const pyas_comoments &b) {
        const double na = (double)a.count, nb = (double)b.count;
        const double dx = b.mean_x - a.mean_x, dy = b.mean_y - a.mean_y;
        const double w = nb / (na + nb);
        pyas_comoments r;
        r.count = a.count + b.count;
        r.mean_x = a.mean_x + dx * w;
        r.mean_y = a.mean_y + dy * w;
        r.m2_x = a.m2_x + b.m2_x + dx * dx * na * w;
        r.m2_y = a.m2_y + b.m2_y + dy * dy * na * w;
        r.cxy = a.cxy + b.cxy + dx * dy * na * w;
        if (b.count == 0) r = a;         // an empty side is skipped, not multiplied through
        else if (a.count == 0) r = b;
        return r;
    }
    static __device__ __forceinline__ pyas_comoments shfl_xor(const pyas_comoments &p, int m) {
        pyas_comoments q;
        q.count = pyas::shfl_xor(p.count, m);
        q.mean_x = pyas::shfl_xor(p.mean_x, m);
        q.mean_y = pyas::shfl_xor(p.mean_y, m);
        q.m2_x = pyas::shfl_xor(p.m2_x, m);
        q.m2_y = pyas::shfl_xor(p.m2_y, m);
        q.cxy = pyas::shfl_xor(p.cxy, m);
        return q;
    }
};

struct CoAcc {
    double Kx, Ky, s1x, s1y, s2x, s2y, sxy;
    uint32_t n;
    __device__ __forceinline__ void init() {
        Kx = 0.0; Ky = 0.0; s1x = 0.0; s1y = 0.0; s2x = 0.0; s2y = 0.0; sxy = 0.0; n = 0;
    }
    __device__ __forceinline__ void add_d(double dx, double dy, bool ok) {
        s1x += dx;
        s1y += dy;
        s2x = __builtin_fma(dx, dx, s2x);
        s2y = __builtin_fma(dy, dy, s2y);
        sxy = __builtin_fma(dx, dy, sxy);
        n += ok ? 1u : 0u;
    }
    // one pair; ok = selected and unmasked on both sides
    __device__ __forceinline__ void add_one(double x, double y, bool ok) {
        const bool first = ok && n == 0;
        Kx = first ? x : Kx;
        Ky = first ? y : Ky;
        add_d(ok ? x - Kx : 0.0, ok ? y - Ky : 0.0, ok);
    }
    // the shifts are set (n > 0)
    __device__ __forceinline__ void add_next(double x, double y, bool ok) {
        add_d(ok ? x - Kx : 0.0, ok ? y - Ky : 0.0, ok);
    }
    template <int M, typename T>
    static __device__ __forceinline__ bool pair_ok(T x, T y, const MaskT<T> &mkx, const MaskT<T> &mky) {
        if constexpr (M == 0) return true;
        const bool bx = mkx.template masked_m<M>(x), by = mky.template masked_m<M>(y);
        return !(bx | by);
    }
    // N pairs; M: mask mode of both sides (0 none, kMaskRange, kMaskAll).  Once
    // every lane that runs this call has its shifts, they are no longer looked for.
    template <int N, int M, typename T>
    __device__ __forceinline__ void add_n(const T *x, const T *y, const MaskT<T> &mkx, const MaskT<T> &mky) {
        if (__builtin_expect(__ballot(n == 0) != 0, 0)) {
#pragma unroll
            for (int k = 0; k < N; ++k) add_one((double)x[k], (double)y[k], pair_ok<M>(x[k], y[k], mkx, mky));
        } else {
#pragma unroll
            for (int k = 0; k < N; ++k) add_next((double)x[k], (double)y[k], pair_ok<M>(x[k], y[k], mkx, mky));
        }
    }
    __device__ __forceinline__ pyas_comoments finish() const {
        pyas_comoments p;
        if (n == 0) {
            p.count = 0; p.mean_x = 0.0; p.mean_y = 0.0; p.m2_x = 0.0; p.m2_y = 0.0; p.cxy = 0.0;
        } else {
            const double mux = s1x / (double)n, muy = s1y / (double)n;
            const double m2x = __builtin_fma(-s1x, mux, s2x), m2y = __builtin_fma(-s1y, muy, s2y);
            const double c = __builtin_fma(-s1x, muy, sxy);
            p.count = (int64_t)n;
            p.mean_x = Kx + mux;
            p.mean_y = Ky + muy;
            p.m2_x = m2x < 0.0 ? 0.0 : m2x;   // a rounding residue; NaN stays NaN
            p.m2_y = m2y < 0.0 ? 0.0 : m2y;
            // not clamped.  A NaN m2 (an unmasked NaN or +-inf on that side) makes
            // every (x - mean) NaN or infinite with a NaN among them: cxy is NaN
            p.cxy = (m2x != m2x || m2y != m2y) ? __builtin_nan("") : c;
        }
        return p;
    }
};

}  // namespace pyas
