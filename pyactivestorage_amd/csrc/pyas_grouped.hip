// pyas_grouped.hip — per-label second moments behind Active.grouped
// (pyas_group_cols and pyas_group_axes of include/pyas.h).
//
// The pyas_moments record of pyas_moments.hip (count / mean / m2, MomAcc per
// lane, MomMerge above a lane), one record per (output, label): an element at
// global index i along one reduced dim belongs to group labels[i] >= 0, or to
// none (labels[i] < 0: it is never read on the dense path, never counted on
// the walk).
//
// k_group_cols : the dense path, the layout of k_trend_cols.  Unit-step box
//                queries whose reduced dims are a leading prefix of the dims.
//                A workgroup owns 256 items of one column of chunks; an item
//                is kGroupV = 4 consecutive outputs along the innermost dim,
//                aligned to 4 elements of the chunk row.  The host sorts the
//                reduced rows (chunk layer, element offset inside the chunk,
//                label) stably by label, so every group is one run of the
//                list, shared by all columns; rows of no group are not in it.
//                Per pass the workgroup stages kGroupRows rows (the chunk's
//                byte offset, the row's element offset, the label) in LDS; a
//                lane walks them in list order, 4 rows fetched at a time and,
//                for types below 8 bytes, the next 4 rows' loads in flight
//                while these are accumulated.  The label is one LDS broadcast,
//                so "label changed" is uniform over the workgroup: each lane
//                then finishes its 4 accumulators, stores the records at
//                out[g * n_out + o .. o + 3] and starts again (the shift comes
//                from the first counted element of the new run).  The
//                accumulators live across fetch batches and staging passes, so
//                a run may cross either.  The kernel writes EVERY record of
//                its outputs: the all-zero record for a label with no row
//                (skipped between two runs, before the first, behind the
//                last), so `out` needs no zeroing on the stream.  A record is
//                the lane's own sums over all chunk layers: nothing is read
//                back or merged.  Loads as in k_trend_cols (pyas_rows4.hpp):
//                one load of 4 elements where the item lies wholly inside the
//                selection of an aligned chunk, predicated per-element loads
//                otherwise, so padding and unselected elements are never read.
//                Templated on the dtype and shuffled-or-not (18 kernels); byte
//                order is a run-time flag behind one template switch, the mask
//                mode a run-time switch.
// k_group_axes : everything else (strides, index lists, vector mask tables,
//                reduced dims that are not a prefix, every dim reduced): one
//                record per (chunk output, chunk-local group), the reduced
//                walk's digit along the labelled dim going through the group's
//                list of positions among the chunk's selected indices.  A lane
//                per record (innermost dim kept) or a wave per record
//                (innermost dim reduced).  pyas_moments_combine_segments
//                merges the records.  Correct, no speed target.  Templated on
//                the dtype only (10 kernels).
#include <hip/hip_runtime.h>

#include "pyas_moments.hpp"     // MomMerge, MomAcc
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode, axes_extents, rec_wave_merge

namespace pyas {

// ---------------------------------------------------------------------------
// k_group_axes: the per-element walk
// ---------------------------------------------------------------------------
// Positions q0, q0 + stride, ... < n_pos over the dims in `red`, the dim gdim
// counting the glen entries of gp (positions among the selected indices along
// gdim) instead of the dim's whole selection; bo: the kept dims' part.
template <typename T>
__device__ __forceinline__ void gr_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t red, int gdim,
                                        const int32_t *gp, uint32_t glen, const Decomp &bo, int64_t q0, int64_t n_pos,
                                        int64_t stride, bool shuf, bool bsw, const MaskT<T> &mk, MomAcc &acc) {
    for (int64_t q = q0; q < n_pos; q += stride) {
        Decomp od = bo;
        uint32_t e = (uint32_t)q;   // < the chunk's elements < 2^31
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (d < r.ndim && ((red >> d) & 1u)) {
                const uint32_t cd = d == gdim ? glen : (uint32_t)s.cnt[d];
                const uint32_t qq = e / cd;
                int64_t k = e - qq * cd;
                e = qq;
                if (d == gdim) k = gp[k];
                od.mem += sel_index(s, r.pool, d, k) * r.cstride[d];
                od.v[0] += k * r.tab.stride[0][d];
                od.v[1] += k * r.tab.stride[1][d];
            }
        }
        const T x = load_elem_rt<T>(base, r.chunk_elems, od.mem, shuf, bsw);
        acc.add_one((double)x, !all_masked(mk, r.tab, od, x));
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_axes(GroupAxesArgs a) {
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
    int64_t cnt_g = 1;   // the selected extent along gdim
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d == a.gdim) cnt_g = s.cnt[d];
    const int64_t n_rest = cnt_g > 0 ? n_red / cnt_g : 0;   // the other reduced dims' positions
    const int32_t g0 = a.gstart[c];
    const int64_t n_rec = n_keep * (a.gstart[c + 1] - g0);
    pyas_moments *out = a.out + a.out_offsets[c];
    if (!a.row) {   // a lane per record, adjacent lanes at adjacent outputs
        for (int64_t rec = b * kBlock + threadIdx.x; rec < n_rec; rec += a.bpc * kBlock) {
            const int64_t j = rec / n_keep, o = rec - j * n_keep;
            const int32_t p0 = a.gptr[g0 + j], len = a.gptr[g0 + j + 1] - p0;
            MomAcc acc;
            acc.init();
            if (n_rest * len > 0) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                gr_walk<T>(r, base, s, red, a.gdim, a.gpos + p0, (uint32_t)len, bo, 0, n_rest * len, 1, a.shuf, a.bswap,
                           mk, acc);
            }
            out[rec] = acc.finish();
        }
    } else {        // a wave per record (wave-uniform trip count: every lane merges)
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        for (int64_t rec = b * kWaves + threadIdx.x / kWave; rec < n_rec; rec += a.bpc * kWaves) {
            const int64_t j = rec / n_keep, o = rec - j * n_keep;
            const int32_t p0 = a.gptr[g0 + j], len = a.gptr[g0 + j + 1] - p0;
            MomAcc acc;
            acc.init();
            if (lane < n_rest * len) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                gr_walk<T>(r, base, s, red, a.gdim, a.gpos + p0, (uint32_t)len, bo, lane, n_rest * len, kWave, a.shuf,
                           a.bswap, mk, acc);
            }
            pyas_moments p = acc.finish();
            rec_wave_merge<pyas_moments, MomMerge>(p);
            if (lane == 0) out[rec] = p;
        }
    }
}

// ---------------------------------------------------------------------------
// k_group_cols: the dense column walk
// ---------------------------------------------------------------------------
// The rows of one buffer: 4 rows' loads in flight.
template <typename T>
struct GrRows {
    static constexpr int U = 4;
    T v[U][kGroupV];
};

// staged rows q .. q + U - 1 (those below nq) into y; cb: the byte offset of
// each row's chunk, roff: the row's element offset inside it
template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void gr_fetch(const uint8_t *data, int64_t n, int64_t kmem, bool vec_lane, const bool *in,
                                         const int64_t *cb, const int32_t *roff, int q, int nq, GrRows<T> &y) {
    constexpr int U = GrRows<T>::U, V = kGroupV, ES = sizeof(T);
    // 4-element loads: the chunk starts at a multiple of the load's size (and
    // so does every byte plane of a shuffled chunk)
    constexpr int64_t kAlign = (SHUF && ES > 1) ? 4 : (ES * V < 16 ? ES * V : 16);
#pragma unroll
    for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int k = 0; k < V; ++k) y.v[u][k] = (T)0;
        if (q + u < nq) {   // (uniform)
            const uint8_t *base = data + cb[q + u];
            const int64_t i = kmem + roff[q + u];
            if (vec_lane && (((uintptr_t)base & (kAlign - 1)) == 0)) {
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

// The lane's state along the sorted row list.
struct GrLane {
    MomAcc acc[kGroupV];
    int32_t cur;    // the label of the run being accumulated, -1 before the first
    bool hunt;      // some output of the wave still looks for its shift
};

// The run of label ln.cur is over and the next row's label is `next` (the
// group count behind the last run): the finished records of ln.cur, the zero
// records of the labels in between, and fresh accumulators.
__device__ __forceinline__ void gr_advance(GrLane &ln, const bool *in, pyas_moments *out, int64_t n_out, int32_t next) {
    constexpr int V = kGroupV;
    if (ln.cur >= 0) {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (in[k]) out[(int64_t)ln.cur * n_out + k] = ln.acc[k].finish();
    }
    pyas_moments zero;
    zero.count = 0;
    zero.mean = 0.0;
    zero.m2 = 0.0;
    zero.reserved = 0;
    for (int32_t g = ln.cur + 1; g < next; ++g) {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (in[k]) out[(int64_t)g * n_out + k] = zero;
    }
#pragma unroll
    for (int k = 0; k < V; ++k) ln.acc[k].init();
    ln.cur = next;
    ln.hunt = true;
}

// nq staged rows into the lane's state; `in`: which of the 4 outputs are
// selected, vec_lane: all of them and the chunks' rows are a multiple of 4
// elements.  Register double buffer: the next U rows' loads are in flight
// while these U rows are accumulated (8-byte types keep one buffer).
template <typename T, bool SHUF, bool BSW, int M>
__device__ __forceinline__ void gr_rows(const uint8_t *data, int64_t n, int64_t kmem, bool vec_lane, const bool *in,
                                        const int64_t *cb, const int32_t *roff, const int32_t *lab, int nq,
                                        const MaskT<T> &mk, pyas_moments *out, int64_t n_out, GrLane &ln) {
    constexpr int U = GrRows<T>::U, V = kGroupV;
    constexpr bool DB = sizeof(T) < 8;
    GrRows<T> cur, nxt;
    if constexpr (DB) gr_fetch<T, SHUF, BSW>(data, n, kmem, vec_lane, in, cb, roff, 0, nq, cur);
    for (int q = 0; q < nq; q += U) {
        if constexpr (DB) {
            if (q + U < nq) gr_fetch<T, SHUF, BSW>(data, n, kmem, vec_lane, in, cb, roff, q + U, nq, nxt);   // (uniform)
        } else {
            gr_fetch<T, SHUF, BSW>(data, n, kmem, vec_lane, in, cb, roff, q, nq, cur);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (q + u < nq) {   // (uniform)
                const int32_t g = lab[q + u];
                if (g != ln.cur) gr_advance(ln, in, out, n_out, g);   // (uniform over the workgroup)
                // once every output of the wave has its shift it is no longer looked for
                if (__builtin_expect(ln.hunt, 0)) {
                    bool first = false;
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const T v = cur.v[u][k];
                        ln.acc[k].add_one((double)v, in[k] && (M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v)));
                        first |= in[k] && ln.acc[k].n == 0;
                    }
                    ln.hunt = __ballot(first) != 0;
                } else {
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const T v = cur.v[u][k];
                        ln.acc[k].add_next((double)v, in[k] && (M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v)));
                    }
                }
            }
        }
        if constexpr (DB) cur = nxt;
    }
}

template <typename T, bool SHUF, bool BSW>
__device__ __forceinline__ void gr_rows_m(int mode, const uint8_t *data, int64_t n, int64_t kmem, bool vec_lane,
                                          const bool *in, const int64_t *cb, const int32_t *roff, const int32_t *lab,
                                          int nq, const MaskT<T> &mk, pyas_moments *out, int64_t n_out, GrLane &ln) {
    if (mode == 0) gr_rows<T, SHUF, BSW, 0>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
    else if (mode == kMaskRange)
        gr_rows<T, SHUF, BSW, kMaskRange>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
    else gr_rows<T, SHUF, BSW, kMaskAll>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_group_cols(GroupColsArgs a) {
    constexpr int V = kGroupV;
    const ReduceArgs &r = a.r;
    const int nd = r.ndim, P = a.P, L = nd - 1;
    const int64_t col = (int64_t)blockIdx.x / a.bpc, sb = (int64_t)blockIdx.x % a.bpc;
    // The kept dims' selection is the same in every layer of the column: read
    // it from layer 0 (chunk `col`).
    Sel s0;
    load_sel(s0, r.sel, col, nd, r.shape);
    int64_t KO = 1;
#pragma unroll
    for (int d = 0; d < PYAS_MAX_DIMS; ++d)
        if (d >= P && d < L) KO *= s0.cnt[d];
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
    // (as k_trend_cols)
    int64_t kmem = i0, fidx = 0;
    {
        int64_t rest = col, cs = 1;
#pragma unroll
        for (int d = PYAS_MAX_DIMS - 1; d >= 0; --d) {
            if (d < nd && d >= P) {
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
    // (left as a call, init would take the address of the kernel arguments and keep a copy of them in scratch)
    [[clang::always_inline]] mk.init(r.mask);
    const int mode = mask_mode(a.masked, r.mask.flags);
    const bool vec_lane = full && (r.shape[L] % V) == 0;
    __shared__ int64_t s_cb[kGroupRows];
    __shared__ int32_t s_roff[kGroupRows];
    __shared__ int32_t s_lab[kGroupRows];
    GrLane ln;
#pragma unroll
    for (int k = 0; k < V; ++k) ln.acc[k].init();
    ln.cur = -1;
    ln.hunt = true;
    pyas_moments *out = a.out + fidx;   // the lane's 4 outputs are adjacent: the innermost dim's output stride is 1
    for (int64_t t0 = 0; t0 < a.n_rows; t0 += kGroupRows) {
        const int nq = (int)(a.n_rows - t0 < kGroupRows ? a.n_rows - t0 : kGroupRows);
        __syncthreads();   // the previous pass has been read
        for (int q = threadIdx.x; q < nq; q += kBlock) {
            s_cb[q] = r.offsets[(int64_t)a.row_layer[t0 + q] * a.n_cols + col];
            s_roff[q] = a.row_off[t0 + q];
            s_lab[q] = a.row_label[t0 + q];
        }
        __syncthreads();
        if (live) {
            if (a.bswap)
                gr_rows_m<T, SHUF, true>(mode, r.data, r.chunk_elems, kmem, vec_lane, in, s_cb, s_roff, s_lab, nq, mk, out,
                                         a.n_out, ln);
            else
                gr_rows_m<T, SHUF, false>(mode, r.data, r.chunk_elems, kmem, vec_lane, in, s_cb, s_roff, s_lab, nq, mk, out,
                                          a.n_out, ln);
        }
    }
    if (live) gr_advance(ln, in, out, a.n_out, a.n_groups);   // the last run and the labels behind it
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
template <typename T>
hipError_t launch_gr_axes_t(const GroupAxesArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_group_axes<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_group_axes(int dtype, const GroupAxesArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_gr_axes_t, a, grid, st)
}

hipError_t launch_group_cols(int dtype, const GroupColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_group_cols), a, shuf, grid, 0, st)
}

}  // namespace pyas
