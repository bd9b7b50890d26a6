// pyas_moments.hip — second-moment kernels behind Active.var / Active.std
// (pyas_moments_axes and the two moments combines of include/pyas.h).
//
// One pass over the same bytes a mean reads.  Per lane: a shift K (the first
// unmasked value the lane meets, as f64), n, s1 = sum (x-K), s2 = sum (x-K)^2
// in f64 with FMA; a lane finishes to (n, K + s1/n, s2 - s1^2/n).  Everything
// above a lane (lanes of a wave, waves, tiles, chunks, chunk layers) merges
// pyas_moments records with Chan's formula in a fixed order, so a result is
// bit-identical from run to run and does not depend on the launch geometry.
// Masked elements are excluded by select (never multiplied by 0).
//
// k_moments_full : every dim reduced, one workgroup per (chunk, tile).  A whole
//                  chunk or a selection that is one contiguous run streams
//                  16-B loads, register double-buffered, with scalar head and
//                  tail; anything else walks per element.
// k_moments_axes : partial axes, one record per kept output.  Innermost dim
//                  kept: a lane per output (adjacent lanes read adjacent
//                  elements); innermost dim reduced: a wave per output.
// Both are templated on the dtype and shuffled-or-not only; byte order, mask
// rules and selection kind are run-time branches (18 kernels each).
#include <hip/hip_runtime.h>

#include "pyas_moments.hpp"     // MomMerge, MomAcc
#include "pyas_records.hpp"     // the tile / segment / grid combines
#include "pyas_stat_walk.hpp"   // the runs, the offset map, the record merges

namespace pyas {

// (pyas_stat_walk.hpp has this walk for the counting accumulators, which take the 4 elements in
// one call; fed to MomAcc that way the kernels compile to other registers, so the copy stays.)
// Per-element walk of positions q0, q0 + stride, ... < n_pos over the dims in
// `dmask` (rc: the radix counter at q0), 4 loads in flight.
template <typename T, bool SHUF>
__device__ __forceinline__ void mom_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t dmask,
                                         const Decomp &base_o, RadixCounter &rc, int64_t q0, int64_t n_pos,
                                         int64_t stride, bool bsw, const MaskT<T> &mk, MomAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp od[U];
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            od[u] = base_o;
            rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od[u]);
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od[u].mem, bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one((double)x[u], !all_masked(mk, r.tab, od[u], x[u]));
    }
    for (; q < n_pos; q += stride) {
        Decomp od = base_o;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, od);
        rc.advance();
        const T x = load_elem_bsw<T, SHUF>(base, r.chunk_elems, od.mem, bsw);
        acc.add_one((double)x, !all_masked(mk, r.tab, od, x));
    }
}

// The same walk with the reduced positions' element offsets already in LDS (no
// vector mask tables): per element one LDS read, one add, one load.
constexpr int kMomRoff = 4096;   // reduced positions kept in LDS (int32, 16 KiB)
template <typename T, bool SHUF>
__device__ __forceinline__ void mom_walk_lds(const uint8_t *base, int64_t chunk_elems, const int32_t *roff,
                                             int64_t base_mem, int64_t q0, int64_t n_pos, int64_t stride, bool bsw,
                                             const MaskT<T> &mk, MomAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        T x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = load_elem_bsw<T, SHUF>(base, chunk_elems, base_mem + roff[q + u * stride], bsw);
#pragma unroll
        for (int u = 0; u < U; ++u) acc.add_one((double)x[u], !mk.masked(x[u]));
    }
    for (; q < n_pos; q += stride) {
        const T x = load_elem_bsw<T, SHUF>(base, chunk_elems, base_mem + roff[q], bsw);
        acc.add_one((double)x, !mk.masked(x));
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_moments_full(MomentsArgs a) {
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
    MomAcc acc;
    acc.init();
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
            mom_walk<T, SHUF>(r, base, s, all, zero, rc, e0 + threadIdx.x, e1, kBlock, a.bswap, mk, acc);
        }
    }
    rec_store_full<MomMerge>(acc, a, c);
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_moments_axes(MomentsArgs a) {
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
    __shared__ int32_t s_roff[kMomRoff];
    const bool mapped = !(r.tab.on[0] || r.tab.on[1]) && n_red <= kMomRoff;   // uniform
    if (mapped) stage_roff(r, s, red, n_red, s_roff);
    pyas_moments *out = a.out + a.out_offsets[c];
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            MomAcc acc;
            acc.init();
            if (n_red > 0) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    mom_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, 0, n_red, 1, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, 0, 1);
                    mom_walk<T, SHUF>(r, base, s, red, bo, rc, 0, n_red, 1, a.bswap, mk, acc);
                }
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            MomAcc acc;
            acc.init();
            if (lane < n_red) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                if (mapped) {
                    mom_walk_lds<T, SHUF>(base, r.chunk_elems, s_roff, bo.mem, lane, n_red, kWave, a.bswap, mk, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                    mom_walk<T, SHUF>(r, base, s, red, bo, rc, lane, n_red, kWave, a.bswap, mk, acc);
                }
            }
            pyas_moments p = acc.finish();
            rec_wave_merge<pyas_moments, MomMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
hipError_t launch_moments_full(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_moments_full), a, shuf, grid, 0, st)
}

hipError_t launch_moments_axes(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_moments_axes), a, shuf, grid, 0, st)
}

// the combines: pyas_records.hpp over the record and MomMerge
hipError_t launch_moments_tiles(const pyas_moments *tiles, int64_t tpc, int64_t n_chunks,
                                const int64_t *out_offsets, pyas_moments *out, hipStream_t st) {
    return launch_rec_tiles<pyas_moments, MomMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

hipError_t launch_moments_segments(const pyas_moments *in, const int64_t *index, const int64_t *seg,
                                   int64_t n_seg, pyas_moments *out, hipStream_t st) {
    return launch_rec_segments<pyas_moments, MomMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_moments_grid(const pyas_moments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                               pyas_moments *out, hipStream_t st) {
    return launch_rec_grid<pyas_moments, MomMerge>(in, g, n_out, n_layers, out, st);
}

}  // namespace pyas
