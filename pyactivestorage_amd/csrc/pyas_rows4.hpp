// pyas_rows4.hpp — the 4-element row loader of the dense column walks
// (k_trend_cols of pyas_trend.hip, k_group_cols of pyas_grouped.hip): a lane
// owns 4 consecutive outputs along the innermost dim, aligned to 4 elements of
// the chunk row.
#pragma once

#include <hip/hip_runtime.h>

#include "pyas_kernels.hpp"   // ldg16, unpack16

namespace pyas {

// Elements i .. i + 3 of the chunk in one load per byte plane (SHUF) or one
// load of 4 ES bytes (16-B loads for ES >= 4).  The caller has checked the
// alignment and that all four are selected.
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void tr_load4(const uint8_t *base, int64_t n, int64_t i, T *y) {
    constexpr int ES = sizeof(T);
    using U = typename TT<T>::U;
    typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
    if constexpr (SHUF && ES > 1) {
        uint32_t pl[ES];
#pragma unroll
        for (int b = 0; b < ES; ++b)
            pl[b] = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(base + (int64_t)b * n + i));
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            U u = 0;
#pragma unroll
            for (int b = 0; b < ES; ++b) u |= (U)((pl[b] >> (8 * k)) & 0xffu) << (BSW ? 8 * (ES - 1 - b) : 8 * b);
            y[k] = bits_to<T>(u);
        }
    } else if constexpr (ES == 1) {
        const uint32_t w = __builtin_nontemporal_load(reinterpret_cast<const uint32_t *>(base + i));
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = bits_to<T>((uint8_t)(w >> (8 * k)));
    } else if constexpr (ES == 2) {
        const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2 *>(base + i * 2));
        const uint16_t h[4] = {(uint16_t)w.x, (uint16_t)(w.x >> 16), (uint16_t)w.y, (uint16_t)(w.y >> 16)};
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = bits_to<T>(BSW ? bswap(h[k]) : h[k]);
    } else if constexpr (ES == 4) {
        unpack16<T, BSW>(ldg16(reinterpret_cast<const uint4 *>(base + i * 4)), y);
    } else {
        const uint4 *p = reinterpret_cast<const uint4 *>(base + i * 8);
        const uint4 r0 = ldg16(p), r1 = ldg16(p + 1);
        unpack16<T, BSW>(r0, y);
        unpack16<T, BSW>(r1, y + 2);
    }
}

}  // namespace pyas
