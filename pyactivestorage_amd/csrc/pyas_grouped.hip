// pyas_grouped.hip — per-label statistics behind Active.grouped
// (pyas_group_cols / pyas_group_axes and their _partial forms, include/pyas.h).
//
// Two records over the same two walks, the accumulator a template argument:
// MomAcc -> pyas_moments (mean / var / std / count) and PartAcc<T> ->
// pyas_partial (sum / count / min / max).  The walks below are written once;
// k_group_cols and k_group_axes are the MomAcc instances under their old
// names, k_group_cols_partial and k_group_axes_partial the PartAcc ones.
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
// PartAcc<T>   : AccT<T, uint32_t> of pyas_device.hpp per lane: the sum in
//                TT<T>::Acc (f64 from the first addition for floats, int64 /
//                uint64 wrapping for ints), min and max compared in T with
//                pmin / pmax (NaN-propagating), one element per call: a
//                column lane sees one element per row, so there is no f32
//                group of four and no hunt for a shift.  One kernel per dtype
//                carries all four fields (18 + 10 kernels); sum, min and max
//                are picked by pyas_format_partials afterwards.
#include <hip/hip_runtime.h>

#include "pyas_moments.hpp"     // MomMerge, MomAcc
#include "pyas_rows4.hpp"       // tr_load4
#include "pyas_stat_walk.hpp"   // mask_mode, axes_extents, rec_wave_merge

namespace pyas {

// ---------------------------------------------------------------------------
// the two accumulators behind one interface
// ---------------------------------------------------------------------------
// sum / count / min / max of one (output, group) in a lane
template <typename T>
struct PartAcc {
    Acc<T> a;
    __device__ __forceinline__ void init() { a.init(); }
    __device__ __forceinline__ void add(T x, bool ok) { a.add_flag(x, !ok); }
    // (count == 0 leaves sum 0 and the neutral extremes, which merge as nothing)
    __device__ __forceinline__ pyas_partial finish() const {
        pyas_partial p;
        TT<T>::put_acc(p.sum, a.sum);
        p.count = (int64_t)a.count;
        TT<T>::put(p.min, a.mn);
        TT<T>::put(p.max, a.mx);
        return p;
    }
};

template <typename T>
struct PartMerge {
    // a then b (a float sum's last bit depends on the order, so every caller fixes it)
    static __device__ __forceinline__ pyas_partial merged(const pyas_partial &a, const pyas_partial &b) {
        pyas_partial r;
        if constexpr (TT<T>::kind == 0) r.sum.f = a.sum.f + b.sum.f;
        else r.sum.u = a.sum.u + b.sum.u;   // two's complement: the signed sum wraps the same way
        r.count = a.count + b.count;
        TT<T>::put(r.min, pmin(TT<T>::from(a.min), TT<T>::from(b.min)));
        TT<T>::put(r.max, pmax(TT<T>::from(a.max), TT<T>::from(b.max)));
        if (b.count == 0) r = a;         // an empty side is skipped: its extremes mean nothing
        else if (a.count == 0) r = b;
        return r;
    }
    static __device__ __forceinline__ pyas_partial shfl_xor(const pyas_partial &p, int m) {
        pyas_partial q;
        q.sum.u = pyas::shfl_xor(p.sum.u, m);
        q.count = pyas::shfl_xor(p.count, m);
        q.min.u = pyas::shfl_xor(p.min.u, m);
        q.max.u = pyas::shfl_xor(p.max.u, m);
        return q;
    }
};

// What a walk needs to know of its accumulator: the record, its merge, its
// zero, and whether the lane hunts for a shift (MomAcc's K) at a run's start.
template <typename A> struct GrRec;
template <> struct GrRec<MomAcc> {
    using R = pyas_moments;
    using Merge = MomMerge;
    static constexpr bool kHunt = true;
    static __device__ __forceinline__ pyas_moments zero() {
        pyas_moments z;
        z.count = 0;
        z.mean = 0.0;
        z.m2 = 0.0;
        z.reserved = 0;
        return z;
    }
};
template <typename T> struct GrRec<PartAcc<T>> {
    using R = pyas_partial;
    using Merge = PartMerge<T>;
    static constexpr bool kHunt = false;
    static __device__ __forceinline__ pyas_partial zero() {
        pyas_partial z;
        z.sum.u = 0;
        z.count = 0;
        z.min.u = 0;
        z.max.u = 0;
        return z;
    }
};

template <typename T>
__device__ __forceinline__ void gr_add(MomAcc &acc, T x, bool ok) { acc.add_one((double)x, ok); }
template <typename T>
__device__ __forceinline__ void gr_add(PartAcc<T> &acc, T x, bool ok) { acc.add(x, ok); }

// ---------------------------------------------------------------------------
// k_group_axes: the per-element walk
// ---------------------------------------------------------------------------
// Positions q0, q0 + stride, ... < n_pos over the dims in `red`, the dim gdim
// counting the glen entries of gp (positions among the selected indices along
// gdim) instead of the dim's whole selection; bo: the kept dims' part.
template <typename T, typename A>
__device__ __forceinline__ void gr_walk(const ReduceArgs &r, const uint8_t *base, const Sel &s, uint32_t red, int gdim,
                                        const int32_t *gp, uint32_t glen, const Decomp &bo, int64_t q0, int64_t n_pos,
                                        int64_t stride, bool shuf, bool bsw, const MaskT<T> &mk, A &acc) {
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
        gr_add(acc, x, !all_masked(mk, r.tab, od, x));
    }
}

template <typename T, typename A>
__device__ __forceinline__ void group_axes_body(const GroupAxesArgs &a) {
    using R = typename GrRec<A>::R;
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
    R *out = static_cast<R *>(a.out) + a.out_offsets[c];
    if (!a.row) {   // a lane per record, adjacent lanes at adjacent outputs
        for (int64_t rec = b * kBlock + threadIdx.x; rec < n_rec; rec += a.bpc * kBlock) {
            const int64_t j = rec / n_keep, o = rec - j * n_keep;
            const int32_t p0 = a.gptr[g0 + j], len = a.gptr[g0 + j + 1] - p0;
            A acc;
            acc.init();
            if (n_rest * len > 0) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                gr_walk<T, A>(r, base, s, red, a.gdim, a.gpos + p0, (uint32_t)len, bo, 0, n_rest * len, 1, a.shuf, a.bswap,
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
            A acc;
            acc.init();
            if (lane < n_rest * len) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                gr_walk<T, A>(r, base, s, red, a.gdim, a.gpos + p0, (uint32_t)len, bo, lane, n_rest * len, kWave, a.shuf,
                           a.bswap, mk, acc);
            }
            R p = acc.finish();
            rec_wave_merge<R, typename GrRec<A>::Merge>(p);
            if (lane == 0) out[rec] = p;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_axes(GroupAxesArgs a) {
    group_axes_body<T, MomAcc>(a);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void k_group_axes_partial(GroupAxesArgs a) {
    group_axes_body<T, PartAcc<T>>(a);
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
template <typename A>
struct GrLane {
    A acc[kGroupV];
    int32_t cur;    // the label of the run being accumulated, -1 before the first
    bool hunt;      // some output of the wave still looks for its shift (MomAcc only)
};

// The run of label ln.cur is over and the next row's label is `next` (the
// group count behind the last run): the finished records of ln.cur, the zero
// records of the labels in between, and fresh accumulators.
template <typename A>
__device__ __forceinline__ void gr_advance(GrLane<A> &ln, const bool *in, typename GrRec<A>::R *out, int64_t n_out,
                                           int32_t next) {
    constexpr int V = kGroupV;
    if (ln.cur >= 0) {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (in[k]) out[(int64_t)ln.cur * n_out + k] = ln.acc[k].finish();
    }
    const typename GrRec<A>::R zero = GrRec<A>::zero();
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
template <typename T, bool SHUF, bool BSW, int M, typename A>
__device__ __forceinline__ void gr_rows(const uint8_t *data, int64_t n, int64_t kmem, bool vec_lane, const bool *in,
                                        const int64_t *cb, const int32_t *roff, const int32_t *lab, int nq,
                                        const MaskT<T> &mk, typename GrRec<A>::R *out, int64_t n_out, GrLane<A> &ln) {
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
                if constexpr (!GrRec<A>::kHunt) {   // no shift: every element goes the same way
#pragma unroll
                    for (int k = 0; k < V; ++k) {
                        const T v = cur.v[u][k];
                        gr_add(ln.acc[k], v, in[k] && (M == 0 || !mk.template masked_m<M ? M : kMaskAll>(v)));
                    }
                // once every output of the wave has its shift it is no longer looked for
                } else if (__builtin_expect(ln.hunt, 0)) {
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

template <typename T, bool SHUF, bool BSW, typename A>
__device__ __forceinline__ void gr_rows_m(int mode, const uint8_t *data, int64_t n, int64_t kmem, bool vec_lane,
                                          const bool *in, const int64_t *cb, const int32_t *roff, const int32_t *lab,
                                          int nq, const MaskT<T> &mk, typename GrRec<A>::R *out, int64_t n_out,
                                          GrLane<A> &ln) {
    if (mode == 0) gr_rows<T, SHUF, BSW, 0>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
    else if (mode == kMaskRange)
        gr_rows<T, SHUF, BSW, kMaskRange>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
    else gr_rows<T, SHUF, BSW, kMaskAll>(data, n, kmem, vec_lane, in, cb, roff, lab, nq, mk, out, n_out, ln);
}

// (the body is included, not called: see pyas_group_cols_body.inc)
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_group_cols(GroupColsArgs a) {
    using A = MomAcc;
#include "pyas_group_cols_body.inc"
}

template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_group_cols_partial(GroupColsArgs a) {
    using A = PartAcc<T>;
#include "pyas_group_cols_body.inc"
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

template <typename T>
hipError_t launch_gr_axes_partial_t(const GroupAxesArgs &a, int64_t grid, hipStream_t st) {
    hipLaunchKernelGGL((k_group_axes_partial<T>), dim3((unsigned)grid), dim3(kBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_group_axes_partial(int dtype, const GroupAxesArgs &a, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_gr_axes_partial_t, a, grid, st)
}

hipError_t launch_group_cols_partial(int dtype, const GroupColsArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_group_cols_partial), a, shuf, grid, 0, st)
}

}  // namespace pyas
