// pyas_records.hpp — the three combines of f64 records, written over the
// record and its merge.  The second moments (pyas_moments.hip, 32 bytes), the
// weighted sums (pyas_weighted.hip, 32 bytes) and the co-moments
// (pyas_comoments.hip, 48 bytes; pyas_trend.hip's records too) use them.
// One thread per output folds its records sequentially in a fixed order: tiles
// in tile order, a segment in index order (pyas_combine_segments), chunk layers
// in C order over the reduced dims' chunk coordinates (pyas_combine_grid).
//
// R is the record (the all-zero record is neutral); M::merged(a, b) merges a
// then b (the order matters to the last bit, so every caller fixes it).
#pragma once

#include "pyas_internal.hpp"

namespace pyas {

template <typename R, typename M>
__global__ __launch_bounds__(kBlock) void k_rec_tiles(const R *tiles, int64_t tpc, int64_t n_chunks,
                                                      const int64_t *out_offsets, R *out) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= n_chunks) return;
    R p = tiles[c * tpc];
    for (int64_t t = 1; t < tpc; ++t) p = M::merged(p, tiles[c * tpc + t]);
    out[out_offsets ? out_offsets[c] : c] = p;
}

// U records in flight, merged in index order (fewer for a large record)
template <typename R, typename M, int U = 8>
__global__ __launch_bounds__(kBlock) void k_rec_segments(const R *in, const int64_t *index, const int64_t *seg,
                                                         int64_t n_seg, R *out) {
    const int64_t sidx = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (sidx >= n_seg) return;
    R p{};
    const int64_t k1 = seg[sidx + 1];
    for (int64_t k0 = seg[sidx]; k0 < k1; k0 += U) {
        R q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            q[u] = R{};
            if (k0 + u < k1) q[u] = in[index ? index[k0 + u] : k0 + u];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) p = M::merged(p, q[u]);
    }
    out[sidx] = p;
}

// the walk of k_combine_grid: output f's kept coordinates give the chunk
// position and the index j in each chunk's record array; the layers follow in
// C order over the reduced dims' chunk coordinates
template <typename R, typename M>
__global__ __launch_bounds__(kBlock) void k_rec_grid(const R *in, pyas_grid g, int64_t n_out, int64_t n_layers,
                                                     R *out) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= n_out) return;
    int64_t gstride[PYAS_MAX_DIMS], digit[PYAS_MAX_DIMS];
    int64_t j = 0, jstride = 1, st = 1, n = 0, rest = f;
#pragma unroll
    for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
        gstride[d] = st;
        digit[d] = 0;
        if (d < g.ndim) {
            if (!((g.axes_mask >> d) & 1u)) {
                const int64_t e = g.out_extent[d];
                const int64_t p = rest % e;
                rest /= e;
                const int64_t ad = g.pos_coord[d][p];
                n += ad * st;
                j += (int64_t)g.pos_local[d][p] * jstride;
                jstride *= g.coord_count[d][ad];
            }
            st *= g.n_coords[d];
        }
    }
    R p{};
    for (int64_t l = 0; l < n_layers; ++l) {
        const int64_t off = g.chunk_out_offsets[n];
        bool carry = true;
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (carry && d < g.ndim && ((g.axes_mask >> d) & 1u)) {
                n += gstride[d];
                if (++digit[d] == g.n_coords[d]) {
                    digit[d] = 0;
                    n -= g.n_coords[d] * gstride[d];
                } else {
                    carry = false;
                }
            }
        }
        p = M::merged(p, in[off + j]);
    }
    out[f] = p;
}

template <typename R, typename M>
hipError_t launch_rec_tiles(const R *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets, R *out,
                            hipStream_t st) {
    const int64_t nb = (n_chunks + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((k_rec_tiles<R, M>), dim3((unsigned)nb), dim3(kBlock), 0, st, tiles, tpc, n_chunks,
                       out_offsets, out);
    return hipGetLastError();
}

template <typename R, typename M, int U = 8>
hipError_t launch_rec_segments(const R *in, const int64_t *index, const int64_t *seg, int64_t n_seg, R *out,
                               hipStream_t st) {
    const int64_t nb = (n_seg + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((k_rec_segments<R, M, U>), dim3((unsigned)nb), dim3(kBlock), 0, st, in, index, seg, n_seg, out);
    return hipGetLastError();
}

template <typename R, typename M>
hipError_t launch_rec_grid(const R *in, const pyas_grid &g, int64_t n_out, int64_t n_layers, R *out,
                           hipStream_t st) {
    const int64_t nb = (n_out + kBlock - 1) / kBlock;
    hipLaunchKernelGGL((k_rec_grid<R, M>), dim3((unsigned)nb), dim3(kBlock), 0, st, in, g, n_out, n_layers, out);
    return hipGetLastError();
}

}  // namespace pyas
