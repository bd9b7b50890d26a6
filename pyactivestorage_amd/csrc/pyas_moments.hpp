// pyas_moments.hpp — the second-moment record's merge and accumulator,
// shared by pyas_moments.hip (Active.var / Active.std) and pyas_grouped.hip
// (Active.grouped: one record per label).
#pragma once

#include "pyas_device.hpp"   // MaskT, shfl_xor

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
    static __device__ __forceinline__ pyas_moments shfl_xor(const pyas_moments &p, int m) {
        pyas_moments q;
        q.count = pyas::shfl_xor(p.count, m);
        q.mean = pyas::shfl_xor(p.mean, m);
        q.m2 = pyas::shfl_xor(p.m2, m);
        q.reserved = 0;
        return q;
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

}  // namespace pyas
