// pyas_comoments.hip — co-moment kernels behind Active.cov / Active.corr
// (pyas_comoments_axes and the two comoments combines of include/pyas.h).
//
// The two-variable sibling of pyas_moments.hip: one pass over the bytes the
// two var passes read.  Chunk c of y pairs with chunk c of x under x's
// selection; a pair counts when it is unmasked on both sides (each side its
// own mask).  Per lane: shifts Kx, Ky (the lane's first counted pair, as f64),
// n, s1x = sum (x-Kx), s1y, s2x = sum (x-Kx)^2, s2y, sxy = sum (x-Kx)(y-Ky) in
// f64 with FMA; a lane finishes to (n, Kx + s1x/n, Ky + s1y/n, s2x - s1x^2/n,
// s2y - s1y^2/n, sxy - s1x s1y/n).  Everything above a lane merges
// pyas_comoments records with Chan's formula in the fixed order of the moments
// records, so a result is bit-identical from run to run.  Masked or unpaired
// elements are excluded by select (never multiplied by 0).
//
// k_comoments_full : every dim reduced, one workgroup per (chunk, tile).  A
//                    selection that is one contiguous run streams both buffers
//                    with 16-B loads, register double-buffered (2 vectors per
//                    stream in flight twice: the registers of k_moments_full's
//                    4), when both chunk bases are misaligned alike; a shuffled
//                    side turns the run into groups of 16 elements (its byte
//                    planes against 16 plain elements of the other side);
//                    anything else walks per element.  Templated on the dtype
//                    and each side's shuffle (34 kernels).
// k_comoments_axes : partial axes, one record per kept output; a lane per
//                    output (innermost dim kept) or a wave per output.  The
//                    reduced positions' offsets sit in LDS when they fit: one
//                    table for both variables.  Templated on the dtype only:
//                    its loads are per element, so each side's shuffle is a
//                    run-time branch (10 kernels).
// Byte order, mask rules and selection kind are run-time branches.
#include <hip/hip_runtime.h>

#include "pyas_records.hpp"     // the three combines over a record and its merge
#include "pyas_comoments.hpp"   // ComomMerge, CoAcc
#include "pyas_stat_walk.hpp"   // the tile share, the offset map, the record merges

namespace pyas {

// RT: some side is byte-swapped (a run-time flag per side); else no branch
template <typename T, bool RT>
__device__ __forceinline__ void com_unpack(const uint4 &r, T *x, bool bsw) {
    if constexpr (RT) {
        if (bsw) unpack16<T, true>(r, x);
        else unpack16<T, false>(r, x);
    } else {
        unpack16<T, false>(r, x);
    }
}

// ---------------------------------------------------------------------------
// contiguous runs: chunk elements [m0, m1) of both buffers
// ---------------------------------------------------------------------------
template <typename T, bool SX, bool SY, int M>
__device__ __forceinline__ void com_run_elems(const uint8_t *bx, const uint8_t *by, int64_t n, int64_t i0, int64_t i1,
                                              bool bsx, bool bsy, CoAcc &acc, const MaskT<T> &mkx,
                                              const MaskT<T> &mky) {
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kBlock) {
        const T x = load_elem_bsw<T, SX>(bx, n, i, bsx), y = load_elem_bsw<T, SY>(by, n, i, bsy);
        acc.template add_n<1, M>(&x, &y, mkx, mky);
    }
}

// Both sides plain (the layout of stat_run_plain): the vector path needs the
// same head and tail on both sides, i.e. bases misaligned alike.
template <typename T, int M, bool RT>
__device__ void com_run_plain(const uint8_t *bx, const uint8_t *by, int64_t m0, int64_t m1, bool bsx, bool bsy,
                              CoAcc &acc, const MaskT<T> &mkx, const MaskT<T> &mky) {
    constexpr int ES = sizeof(T);
    constexpr int N = 16 / ES;
    const int tid = threadIdx.x;
    const int64_t b0 = m0 * ES, b1 = m1 * ES;               // byte range in the chunk
    const int64_t mis = (int64_t)((uintptr_t)bx & 15);
    const int64_t a0 = ((b0 + mis + 15) & ~(int64_t)15) - mis;  // first 16-B aligned byte
    const int64_t a1 = ((b1 + mis) & ~(int64_t)15) - mis;
    if (mis != (int64_t)((uintptr_t)by & 15) || a0 >= a1) {
        com_run_elems<T, false, false, M>(bx, by, 0, m0, m1, bsx, bsy, acc, mkx, mky);
        return;
    }
    const int64_t nhead = (a0 - b0) / ES, ntail = (b1 - a1) / ES;
    if (tid < nhead) {
        const T x = load_elem_bsw<T, false>(bx, 0, m0 + tid, bsx), y = load_elem_bsw<T, false>(by, 0, m0 + tid, bsy);
        acc.template add_n<1, M>(&x, &y, mkx, mky);
    }
    if (tid < ntail) {
        const int64_t i = m1 - ntail + tid;
        const T x = load_elem_bsw<T, false>(bx, 0, i, bsx), y = load_elem_bsw<T, false>(by, 0, i, bsy);
        acc.template add_n<1, M>(&x, &y, mkx, mky);
    }
    const uint4 *vx = reinterpret_cast<const uint4 *>(bx + a0);
    const uint4 *vy = reinterpret_cast<const uint4 *>(by + a0);
    const int64_t nvec = (a1 - a0) / 16;
    constexpr int U = 2;   // per stream: the two streams hold k_moments_full's 4 + 4 vectors
    constexpr int64_t STEP = (int64_t)U * kBlock;
    const int64_t nsteps = nvec / STEP;
    auto consume = [&](const uint4 *rx, const uint4 *ry) {
#pragma unroll
        for (int u = 0; u < U; ++u) {
            T x[N], y[N];
            com_unpack<T, RT>(rx[u], x, bsx);
            com_unpack<T, RT>(ry[u], y, bsy);
            acc.template add_n<N, M>(x, y, mkx, mky);
        }
    };
    if (nsteps > 0) {
        uint4 cx[U], cy[U], nx[U], ny[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            cx[u] = ldg16(vx + tid + u * kBlock);
            cy[u] = ldg16(vy + tid + u * kBlock);
        }
        for (int64_t s = 0; s + 1 < nsteps; ++s) {
            // the next step's loads are in flight while this step is reduced
#pragma unroll
            for (int u = 0; u < U; ++u) {
                nx[u] = ldg16(vx + (s + 1) * STEP + tid + u * kBlock);
                ny[u] = ldg16(vy + (s + 1) * STEP + tid + u * kBlock);
            }
            consume(cx, cy);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cx[u] = nx[u];
                cy[u] = ny[u];
            }
        }
        consume(cx, cy);
    }
    for (int64_t k = nsteps * STEP + tid; k < nvec; k += kBlock) {
        T x[N], y[N];
        com_unpack<T, RT>(ldg16(vx + k), x, bsx);
        com_unpack<T, RT>(ldg16(vy + k), y, bsy);
        acc.template add_n<N, M>(x, y, mkx, mky);
    }
}

// 16 consecutive elements from element i (a multiple of 16) of one side: the
// ES byte planes of a shuffled chunk, or ES plain 16-B vectors
template <typename T, bool SHUF, bool RT>
__device__ __forceinline__ void com_group16(const uint8_t *base, int64_t n, int64_t i, bool bsw, T *x) {
    constexpr int ES = sizeof(T);
    constexpr int N = 16 / ES;
    uint4 pl[ES];
    if constexpr (SHUF) {
#pragma unroll
        for (int b = 0; b < ES; ++b) pl[b] = ldg16(reinterpret_cast<const uint4 *>(base + (int64_t)b * n + i));
        if constexpr (RT) {
            if (bsw) unshuffle16<T, true>(pl, x);
            else unshuffle16<T, false>(pl, x);
        } else {
            unshuffle16<T, false>(pl, x);
        }
    } else {
#pragma unroll
        for (int b = 0; b < ES; ++b) pl[b] = ldg16(reinterpret_cast<const uint4 *>(base + i * ES) + b);
#pragma unroll
        for (int b = 0; b < ES; ++b) com_unpack<T, RT>(pl[b], x + b * N, bsw);
    }
}

// A shuffled side (or both): elements [i0, i1) in groups of 16 as
// stat_run_shuffled walks them; n = elements in the chunk.
template <typename T, bool SX, bool SY, int M, bool RT>
__device__ void com_run_groups(const uint8_t *bx, const uint8_t *by, int64_t n, int64_t i0, int64_t i1, bool bsx,
                               bool bsy, CoAcc &acc, const MaskT<T> &mkx, const MaskT<T> &mky) {
    const int tid = threadIdx.x;
    // 16-B loads: a shuffled side's planes start at base + b n, a plain side's groups at base + 16 ES g
    const bool okx = (((uintptr_t)bx & 15) == 0) && (!SX || (n & 15) == 0);
    const bool oky = (((uintptr_t)by & 15) == 0) && (!SY || (n & 15) == 0);
    const int64_t g0 = (i0 + 15) & ~(int64_t)15, g1 = i1 & ~(int64_t)15;
    if (!okx || !oky || g0 >= g1) {
        com_run_elems<T, SX, SY, M>(bx, by, n, i0, i1, bsx, bsy, acc, mkx, mky);
        return;
    }
    if (tid < g0 - i0) {
        const T x = load_elem_bsw<T, SX>(bx, n, i0 + tid, bsx), y = load_elem_bsw<T, SY>(by, n, i0 + tid, bsy);
        acc.template add_n<1, M>(&x, &y, mkx, mky);
    }
    if (tid < i1 - g1) {
        const T x = load_elem_bsw<T, SX>(bx, n, g1 + tid, bsx), y = load_elem_bsw<T, SY>(by, n, g1 + tid, bsy);
        acc.template add_n<1, M>(&x, &y, mkx, mky);
    }
    const int64_t ng = (g1 - g0) / 16;
    for (int64_t g = tid; g < ng; g += kBlock) {
        const int64_t i = g0 + g * 16;
        T x[16], y[16];
        com_group16<T, SX, RT>(bx, n, i, bsx, x);
        com_group16<T, SY, RT>(by, n, i, bsy, y);
        acc.template add_n<16, M>(x, y, mkx, mky);
    }
}

template <typename T, bool SX, bool SY, int M, bool RT>
__device__ __forceinline__ void com_run_m(const uint8_t *bx, const uint8_t *by, int64_t n, int64_t i0, int64_t i1,
                                          bool bsx, bool bsy, CoAcc &acc, const MaskT<T> &mkx, const MaskT<T> &mky) {
    if constexpr ((SX || SY) && sizeof(T) > 1)
        com_run_groups<T, SX, SY, M, RT>(bx, by, n, i0, i1, bsx, bsy, acc, mkx, mky);
    else
        com_run_plain<T, M, RT>(bx, by, i0, i1, bsx, bsy, acc, mkx, mky);
}

template <typename T, bool SX, bool SY, bool RT>
__device__ __forceinline__ void com_run(int mode, const uint8_t *bx, const uint8_t *by, int64_t n, int64_t i0,
                                        int64_t i1, bool bsx, bool bsy, CoAcc &acc, const MaskT<T> &mkx,
                                        const MaskT<T> &mky) {
    if (mode == 0) com_run_m<T, SX, SY, 0, RT>(bx, by, n, i0, i1, bsx, bsy, acc, mkx, mky);
    else if (mode == kMaskRange) com_run_m<T, SX, SY, kMaskRange, RT>(bx, by, n, i0, i1, bsx, bsy, acc, mkx, mky);
    else com_run_m<T, SX, SY, kMaskAll, RT>(bx, by, n, i0, i1, bsx, bsy, acc, mkx, mky);
}

// ---------------------------------------------------------------------------
// per-element walks over two buffers
// ---------------------------------------------------------------------------
// How a walk loads and masks each side; the selection and geometry are x's.
struct CoSide {
    const uint8_t *bx, *by;
    bool bsx, bsy, shx, shy;     // shx / shy: only read by the run-time loaders (k_comoments_axes)
    bool ytabs;                  // y has vector mask tables: its table indices are walked too
};

// the table indices of y's vector masks at the radix counter's position
__device__ __forceinline__ void com_locate_y(const RadixCounter &rc, const MaskTab &ty, int ndim, uint32_t dmask,
                                             Decomp &o) {
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
        if (d < ndim && ((dmask >> d) & 1u)) {
            o.v[0] += (int64_t)rc.idx[d] * ty.stride[0][d];
            o.v[1] += (int64_t)rc.idx[d] * ty.stride[1][d];
        }
    }
}

// LX: 0 plain, 1 shuffled, 2 run-time (cs.shx); the same for LY
template <typename T, int L>
__device__ __forceinline__ T com_load_l(const uint8_t *base, int64_t n, int64_t i, bool shuf, bool bsw) {
    if constexpr (L == 2) return load_elem_rt<T>(base, n, i, shuf && sizeof(T) > 1, bsw);
    else return load_elem_bsw<T, L == 1>(base, n, i, bsw);
}

// Positions q0, q0 + stride, ... < n_pos over the dims in `dmask` (rc: the
// radix counter at q0); box / boy: the kept dims' part for x's and y's tables.
template <typename T, int LX, int LY>
__device__ __forceinline__ void com_walk(const ReduceArgs &r, const MaskTab &ty, const CoSide &cs, const Sel &s,
                                         uint32_t dmask, const Decomp &box, const Decomp &boy, RadixCounter &rc,
                                         int64_t q0, int64_t n_pos, int64_t stride, const MaskT<T> &mkx,
                                         const MaskT<T> &mky, CoAcc &acc) {
    constexpr int U = 2;   // pairs: 4 loads in flight
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        Decomp ox[U], oy[U];
        T x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            ox[u] = box;
            oy[u] = boy;
            rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, ox[u]);
            if (cs.ytabs) com_locate_y(rc, ty, r.ndim, dmask, oy[u]);
            rc.advance();
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            x[u] = com_load_l<T, LX>(cs.bx, r.chunk_elems, ox[u].mem, cs.shx, cs.bsx);
            y[u] = com_load_l<T, LY>(cs.by, r.chunk_elems, ox[u].mem, cs.shy, cs.bsy);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const bool mx = all_masked(mkx, r.tab, ox[u], x[u]), my = all_masked(mky, ty, oy[u], y[u]);
            acc.add_one((double)x[u], (double)y[u], !(mx | my));
        }
    }
    for (; q < n_pos; q += stride) {
        Decomp ox = box, oy = boy;
        rc.locate(s, r.pool, r.cstride, r.tab, r.ndim, dmask, ox);
        if (cs.ytabs) com_locate_y(rc, ty, r.ndim, dmask, oy);
        rc.advance();
        const T x = com_load_l<T, LX>(cs.bx, r.chunk_elems, ox.mem, cs.shx, cs.bsx);
        const T y = com_load_l<T, LY>(cs.by, r.chunk_elems, ox.mem, cs.shy, cs.bsy);
        const bool mx = all_masked(mkx, r.tab, ox, x), my = all_masked(mky, ty, oy, y);
        acc.add_one((double)x, (double)y, !(mx | my));
    }
}

// The same walk with the reduced positions' element offsets already in LDS (no
// vector mask tables on either side): one table serves both variables.
constexpr int kComRoff = 4096;   // reduced positions kept in LDS (int32, 16 KiB)
template <typename T>
__device__ __forceinline__ void com_walk_lds(const CoSide &cs, int64_t chunk_elems, const int32_t *roff,
                                             int64_t base_mem, int64_t q0, int64_t n_pos, int64_t stride,
                                             const MaskT<T> &mkx, const MaskT<T> &mky, CoAcc &acc) {
    constexpr int U = 4;
    int64_t q = q0;
    for (; q + (U - 1) * stride < n_pos; q += U * stride) {
        T x[U], y[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t i = base_mem + roff[q + u * stride];
            x[u] = com_load_l<T, 2>(cs.bx, chunk_elems, i, cs.shx, cs.bsx);
            y[u] = com_load_l<T, 2>(cs.by, chunk_elems, i, cs.shy, cs.bsy);
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
            acc.add_one((double)x[u], (double)y[u], CoAcc::pair_ok<kMaskAll>(x[u], y[u], mkx, mky));
    }
    for (; q < n_pos; q += stride) {
        const int64_t i = base_mem + roff[q];
        const T x = com_load_l<T, 2>(cs.bx, chunk_elems, i, cs.shx, cs.bsx);
        const T y = com_load_l<T, 2>(cs.by, chunk_elems, i, cs.shy, cs.bsy);
        acc.add_one((double)x, (double)y, CoAcc::pair_ok<kMaskAll>(x, y, mkx, mky));
    }
}

// ---------------------------------------------------------------------------
// every dim reduced: workgroup = tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SX, bool SY>
__global__ __launch_bounds__(kBlock) void k_comoments_full(ComomentsArgs a) {
    const ReduceArgs &r = a.x;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, t = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *bx = a.x.data + a.x.offsets[c];
    const uint8_t *by = a.y.data + a.y.offsets[c];
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mkx, mky;
    mkx.init(a.x.mask);
    mky.init(a.y.mask);
    const bool ytabs = a.y.tab.on[0] || a.y.tab.on[1];
    const bool tabs = r.tab.on[0] || r.tab.on[1] || ytabs;
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
    CoAcc acc;
    acc.init();
    if (e0 < e1) {
        if (contig) {
            // one mode for both sides: the wider of the two (a rule a side does
            // not have compares against its neutral thresholds)
            const int mx = mask_mode(a.masked_x, a.x.mask.flags), my = mask_mode(a.masked_y, a.y.mask.flags);
            const int mode = (mx == kMaskAll || my == kMaskAll) ? kMaskAll : (mx | my);
            if (a.bswap_x || a.bswap_y)
                com_run<T, SX, SY, true>(mode, bx, by, r.chunk_elems, m0 + e0, m0 + e1, a.bswap_x, a.bswap_y, acc,
                                         mkx, mky);
            else
                com_run<T, SX, SY, false>(mode, bx, by, r.chunk_elems, m0 + e0, m0 + e1, false, false, acc, mkx, mky);
        } else if (e0 + threadIdx.x < e1) {
            const uint32_t all = (1u << r.ndim) - 1u;
            RadixCounter rc;
            rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
            const Decomp zero{0, {0, 0}};
            const CoSide cs{bx, by, a.bswap_x, a.bswap_y, SX, SY, ytabs};
            com_walk<T, SX ? 1 : 0, SY ? 1 : 0>(r, a.y.tab, cs, s, all, zero, zero, rc, e0 + threadIdx.x, e1, kBlock,
                                                mkx, mky, acc);
        }
    }
    rec_store_full<ComomMerge>(acc, a, c);
}

// ---------------------------------------------------------------------------
// partial axes: out[out_offsets[c] + o], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void k_comoments_axes(ComomentsArgs a) {
    const ReduceArgs &r = a.x;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mkx, mky;
    mkx.init(a.x.mask);
    mky.init(a.y.mask);
    const bool ytabs = a.y.tab.on[0] || a.y.tab.on[1];
    const CoSide cs{a.x.data + a.x.offsets[c], a.y.data + a.y.offsets[c], a.bswap_x, a.bswap_y, a.shuf_x, a.shuf_y,
                    ytabs};
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep = 1, n_red = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d) {
        if (d < r.ndim) {
            if ((red >> d) & 1u) n_red *= s.cnt[d];
            else n_keep *= s.cnt[d];
        }
    }
    // the reduced positions' offsets, once per workgroup, when they fit
    __shared__ int32_t s_roff[kComRoff];
    const bool mapped = !(r.tab.on[0] || r.tab.on[1] || ytabs) && n_red <= kComRoff;   // uniform
    if (mapped) stage_roff(r, s, red, n_red, s_roff);
    pyas_comoments *out = a.out + a.out_offsets[c];
    auto kept_part = [&](int64_t o, Decomp &box, Decomp &boy) {
        box = Decomp{0, {0, 0}};
        boy = Decomp{0, {0, 0}};
        decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, box);
        if (ytabs) decompose(s, r.pool, r.cstride, a.y.tab, r.ndim, keep, o, boy);
    };
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            CoAcc acc;
            acc.init();
            if (n_red > 0) {
                Decomp box, boy;
                kept_part(o, box, boy);
                if (mapped) {
                    com_walk_lds<T>(cs, r.chunk_elems, s_roff, box.mem, 0, n_red, 1, mkx, mky, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, 0, 1);
                    com_walk<T, 2, 2>(r, a.y.tab, cs, s, red, box, boy, rc, 0, n_red, 1, mkx, mky, acc);
                }
            }
            out[o] = acc.finish();
        }
    } else {        // a wave per output (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t o = b * kWaves + threadIdx.x / kWave; o < n_keep; o += a.bpc * kWaves) {
            CoAcc acc;
            acc.init();
            if (lane < n_red) {
                Decomp box, boy;
                kept_part(o, box, boy);
                if (mapped) {
                    com_walk_lds<T>(cs, r.chunk_elems, s_roff, box.mem, lane, n_red, kWave, mkx, mky, acc);
                } else {
                    RadixCounter rc;
                    rc.init(s, r.ndim, red, (uint64_t)lane, (uint64_t)kWave);
                    com_walk<T, 2, 2>(r, a.y.tab, cs, s, red, box, boy, rc, lane, n_red, kWave, mkx, mky, acc);
                }
            }
            pyas_comoments p = acc.finish();
            rec_wave_merge<pyas_comoments, ComomMerge>(p);
            if (lane == 0) out[o] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_com_full_t(const ComomentsArgs &a, int64_t grid, hipStream_t st) {
    const dim3 g((unsigned)grid), b(kBlock);
    if constexpr (sizeof(T) > 1) {
        if (a.shuf_x && a.shuf_y) hipLaunchKernelGGL((k_comoments_full<T, true, true>), g, b, 0, st, a);
        else if (a.shuf_x) hipLaunchKernelGGL((k_comoments_full<T, true, false>), g, b, 0, st, a);
        else if (a.shuf_y) hipLaunchKernelGGL((k_comoments_full<T, false, true>), g, b, 0, st, a);
        else hipLaunchKernelGGL((k_comoments_full<T, false, false>), g, b, 0, st, a);
    } else {
        hipLaunchKernelGGL((k_comoments_full<T, false, false>), g, b, 0, st, a);
    }
    return hipGetLastError();
}

template <typename T>
hipError_t launch_com_axes_t(const ComomentsArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_comoments_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_comoments_full(int dtype, const ComomentsArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_com_full_t, a, grid, st)
}

hipError_t launch_comoments_axes(int dtype, const ComomentsArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_com_axes_t, a, grid, st)
}

hipError_t launch_comoments_tiles(const pyas_comoments *tiles, int64_t tpc, int64_t n_chunks,
                                  const int64_t *out_offsets, pyas_comoments *out, hipStream_t st) {
    return launch_rec_tiles<pyas_comoments, ComomMerge>(tiles, tpc, n_chunks, out_offsets, out, st);
}

hipError_t launch_comoments_segments(const pyas_comoments *in, const int64_t *index, const int64_t *seg,
                                     int64_t n_seg, pyas_comoments *out, hipStream_t st) {
    return launch_rec_segments<pyas_comoments, ComomMerge>(in, index, seg, n_seg, out, st);
}

hipError_t launch_comoments_grid(const pyas_comoments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                                 pyas_comoments *out, hipStream_t st) {
    return launch_rec_grid<pyas_comoments, ComomMerge>(in, g, n_out, n_layers, out, st);
}

}  // namespace pyas
