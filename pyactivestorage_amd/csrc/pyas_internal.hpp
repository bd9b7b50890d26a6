// pyas_internal.hpp — kernel argument blocks and launcher prototypes shared by
// pyas_kernels.hip (device code) and pyas_capi.hip (the extern "C" boundary).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <type_traits>

#include "pyas.h"
#include "pyas_device.hpp"

namespace pyas {

// The statistics' launchers (host code).  PYAS_DISPATCH_DTYPE returns
// FN<T>(...) for the element type T of the `dtype` in scope.
#define PYAS_DISPATCH_DTYPE(FN, ...)                                 \
    switch (dtype) {                                                 \
        case PYAS_I8: return FN<int8_t>(__VA_ARGS__);                \
        case PYAS_U8: return FN<uint8_t>(__VA_ARGS__);               \
        case PYAS_I16: return FN<int16_t>(__VA_ARGS__);              \
        case PYAS_U16: return FN<uint16_t>(__VA_ARGS__);             \
        case PYAS_I32: return FN<int32_t>(__VA_ARGS__);              \
        case PYAS_U32: return FN<uint32_t>(__VA_ARGS__);             \
        case PYAS_I64: return FN<int64_t>(__VA_ARGS__);              \
        case PYAS_U64: return FN<uint64_t>(__VA_ARGS__);             \
        case PYAS_F32: return FN<float>(__VA_ARGS__);                \
        case PYAS_F64: return FN<double>(__VA_ARGS__);               \
        default: return hipErrorInvalidValue;                        \
    }

// A kernel template K<T, SHUF> as a value launch_shuf can instantiate.
#define PYAS_SHUF_KERNEL(K) [](auto t, auto s) { return (&K<decltype(t), decltype(s)::value>); }

// K<T, true> over shuffled data of a dtype wider than a byte (one byte has
// nothing to unshuffle: that instantiation does not exist), else K<T, false>.
template <typename T, typename K, typename A>
hipError_t launch_shuf(K kernel, const A &a, bool shuf, int64_t grid, size_t lds, hipStream_t st) {
    if constexpr (sizeof(T) > 1) {
        if (shuf) {
            hipLaunchKernelGGL(kernel(T{}, std::true_type{}), dim3((unsigned)grid), dim3(kBlock), lds, st, a);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL(kernel(T{}, std::false_type{}), dim3((unsigned)grid), dim3(kBlock), lds, st, a);
    return hipGetLastError();
}

// Passed by value in the kernarg segment (a few hundred bytes).
struct ReduceArgs {
    const uint8_t *data;
    const int64_t *offsets;
    const int32_t *sel;
    const int32_t *pool;
    int64_t shape[PYAS_MAX_DIMS];
    int64_t cstride[PYAS_MAX_DIMS];   // row-major element strides of a chunk
    int64_t chunk_elems;
    int64_t tpc;                      // tiles (workgroups) per chunk
    int32_t ndim;
    int32_t spans;                    // run_spans: 0 off, 1 cut chunks run_rows cannot stream, 2 every cut chunk
    pyas_mask mask;
    MaskTab tab;
    pyas_partial *out;                // one partial per workgroup (tile b of chunk b / tpc)
};

// Chunks per first-level combine group: one k_finish block, one thread per
// chunk (k_combine uses the same segments, so both orders agree).
constexpr int64_t kCombineSeg = kBlock;

// k_finish: tile partials -> chunk partials -> group partials -> total
struct FinishArgs {
    const pyas_partial *tiles;        // n_chunks * tpc, chunk-major
    int64_t tpc, n_chunks;
    pyas_partial *chunk_out;          // may be NULL
    pyas_partial *gtmp;               // n_chunks / kCombineSeg + 1 group partials
    pyas_partial *total;              // may be NULL (chunk partials only)
    uint32_t *cnt;                    // zeroed arrival counter; NULL: the host folds gtmp
    uint32_t flags;                   // PYAS_COMBINE_*
};

constexpr int kCutMapWords = 512;   // cut chunks' reduced-position bit map in LDS (16384 positions; + 1 pad word)
constexpr int kAxesLds = 8192;   // reduced-index offsets kept in LDS (int32, 32 KiB)

// Dense partial-axis geometry (k_axes_dense): the chunk dims merged into
// (RO, KO, RI, KI) = (reduced outer, kept outer, reduced inner, kept inner).
constexpr int kSlabBytes = 16384;     // k_axes_shuf_slab: LDS tile per wave (plain elements)

struct AxesDense {
    int32_t mode;                     // 0 off, 1 column, 2 row, 3 row with 4 outputs per lane,
                                      // 4/5/6 row through LDS with 1/2/4 lanes per output
    int32_t it, split;                // column: items per pass (power of 2), row splits
    int32_t group;                    // row: lanes per output (power of 2)
    int64_t RO, KO, RI, KI;
    int64_t bpc;                      // workgroups per chunk of the dense launch
    int64_t cpb;                      // column layout: chunks per workgroup of k_axes_col_stream (0: off)
    int32_t nv;                       // k_axes_col_stream: items per lane (1, 2 or 4)
    int64_t n_chunks;                 // k_axes_col_stream / k_axes_shuf_slab: chunks in the batch
    int64_t rb;                       // k_axes_shuf_slab: rows per LDS tile (0: off)
};

// NumPy's sign of a zero min/max (pyas_tie_*); float types only
struct TieRule {
    int32_t lanes, piece, acc;        // lanes 0: no rule set
    uint8_t rank[64], acc_rank[64];
};
struct AxesArgs {
    ReduceArgs r;
    AxesDense d;
    uint32_t axes;
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;
    pyas_partial *out;
    bool shuf, bswap;
    bool row;                         // innermost dim reduced: G lanes per output
    int32_t group;                    // row layout: lanes per output (power of 2)
    int32_t split;                    // column layout: splits of the reduced range
    bool vec;                         // geometry admits 16-B vector walks (kernel re-checks per chunk)
    int32_t rec;                      // per-chunk outputs: 0 pyas_partial, else a PYAS_REC_* record
    bool cuts;                        // dense launch also takes cut chunks (box, >= half the chunk)
    int32_t zs;                       // the walk keys NumPy's sign of a zero min (1) / max (2)
    TieRule t;                        // zs in the LDS row layout: the host's rule (rows are calls)
    int32_t roff_cap;                 // k_reduce_axes: entries of its LDS offset map (dynamic LDS, <= kAxesLds)
};

// pyas_reduce_axes_grid: the chunk layers of a whole-chunk box query folded
// inside the dense column kernel (no per-chunk partial arrays)
// pyas_combine_grid: internal combine flag (PYAS_COMBINE_WAVE=0) keeping the
// per-thread fold (k_combine_grid) for every layer count
constexpr uint32_t kCombineThreadOnly = 1u << 31;
constexpr int kLeanMaxB = 8;         // k_axes_fold_lean: layers of a split column's second half (LDS sums)
struct FoldGrid;                     // below, after the tie structs it carries


struct InflateArgs {
    const uint8_t *src;
    const int64_t *src_offsets, *src_sizes;
    uint8_t *dst;
    const int64_t *dst_offsets, *dst_capacity;
    int64_t *out_sizes;
    int32_t *status;
};

struct SelectArgs {
    ReduceArgs r;
    int64_t bpc;
    const int64_t *out_offsets;
    void *values;
    uint8_t *mask_out;
    bool shuf, bswap;
    // scatter mode (pyas_select_scatter): element k of chunk c's selection
    // lands at sum_d pos[base[c][d] + k_d] * ostride[d] of the output array
    const int64_t *scatter_pos;
    const int32_t *scatter_base;
    int64_t ostride[PYAS_MAX_DIMS];
};

// Per-dtype launchers: defined in pyas_kernels.hpp, instantiated per dtype by
// pyas_inst.hip.
template <typename T>
hipError_t launch_reduce_t(const ReduceArgs &a, bool shuf, bool bsw, bool masked, int64_t grid,
                           hipStream_t st);
template <typename T>
hipError_t launch_finish_t(const FinishArgs &f, hipStream_t st);
template <typename T>
hipError_t launch_combine_t(const pyas_partial *in, int64_t n, int64_t seg, int64_t nblocks,
                            uint32_t flags, pyas_partial *out, hipStream_t st);
template <typename T>
hipError_t launch_combine_segments_t(const pyas_partial *in, const int64_t *index,
                                     const int64_t *seg, int64_t n_seg, uint32_t flags,
                                     pyas_partial *out, hipStream_t st);
template <typename T>
hipError_t launch_axes_t(const AxesArgs &a, int64_t grid, hipStream_t st);
struct CombineTie;   // below, after the tie structs it carries
template <typename T>
hipError_t launch_combine_grid_t(const pyas_partial *in, const pyas_grid &g, const CombineTie &ct, int64_t n_out,
                                 int64_t n_layers, uint32_t flags, pyas_partial *out,
                                 hipStream_t st);
template <typename T>
hipError_t launch_axes_dense_t(const AxesArgs &a, bool masked, int64_t grid, hipStream_t st);
template <typename T>
hipError_t launch_axes_dense_rows_t(const AxesArgs &a, bool masked, int64_t grid, hipStream_t st);
template <typename T>
hipError_t launch_axes_fold_t(const AxesArgs &a, const FoldGrid &g, bool masked, int64_t grid,
                              hipStream_t st);
template <typename T>
hipError_t launch_axes_fold_rows_t(const AxesArgs &a, const FoldGrid &g, bool masked, int64_t grid,
                                   hipStream_t st);
template <typename T>
hipError_t launch_select_t(const SelectArgs &a, int64_t grid, hipStream_t st);
struct TieCall {
    int32_t acc;                      // 1: strided reduce loop (accumulator keys)
    uint32_t block;                   // acc: kept dims of NumPy's copied first buffer fill
    int64_t lr, npr;                  // call length (1: elementwise), pieces per call
    int64_t n_copy;                   // acc: runs of that fill (contiguous calls), 0: none
};
// k_combine_grid keying level 2 of NumPy's zero sign itself for `out` calls
// of any length (on = 1): the call and the host's rule
struct CombineTie {
    TieCall c;
    TieRule t;
    int32_t on;
};
struct FoldGrid {
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along the reduced dims / kept dims
    uint32_t flags;                   // PYAS_COMBINE_*
    int32_t lean;                     // column layout: k_axes_fold_lean (split 1, rows % 4 == 0),
                                      // 1 = one lane per column item, 2 = layers split over two
    uint32_t zs;                      // NumPy's zero sign fused for min (1) / max (2)
    TieRule t;                        // zs in k_axes_fold_row: the host's rule,
    TieCall c2;                       //   the `out` array's call (level 2), and masks over a
    uint64_t zrow_rem, zrow_top;      //   row's positions e (RI <= 64): remainder, top-priority lane,
    uint64_t zrow_vec, zrow_rep;      //   all lane positions, lane 0's positions (from e = 1),
    uint64_t zrow_cm[64];             //   lane-rank classes (zrow_cm[r]: the lane of rank r)
};
struct TieChunkArgs {
    ReduceArgs r;
    TieRule t;
    pyas_tie_geom g;
    uint32_t axes, which;
    bool shuf, bswap;
    const int64_t *out_offsets;       // NULL: one output per chunk, at index c
    pyas_partial *parts;              // rewrite mode, or NULL and:
    uint8_t *flags;                   //   flag mode (one byte per chunk output)
    const uint32_t *gate;             //   flag mode: skip when *gate == 0
    int64_t n_chunks;
    int32_t cpw;                      // chunks per workgroup: 1, or a wave per chunk (one output each)
    int32_t group;                    // lanes per output: 1, 16 or 64 (k_tie_scan)
    const uint64_t *pick;             // non-NULL (full reductions): only the chunks of the level-2
    TieCall pick_call;                //   K1 / W keys pick[0] / pick[1] (positions pick_base + c
    int64_t pick_base;                //   of the `out` call pick_call), a wave each
};
struct TieGridArgs {
    pyas_grid g;                      // kind 0: layers from the grid tables
    const int64_t *index, *seg;       // kind 1: segments (index NULL: identity)
    int32_t kind;                     // 2: one output, layer l = entry l
    const pyas_partial *parts;        // level-1 partials, or
    const uint8_t *flags;             //   level-1 flag bytes
    pyas_partial *fin;
    uint64_t *keys;
    int64_t n_out, n_layers, layer_base, slices;
    int32_t per_thread;               // k_tie_grid_t: a thread per output (few layers, many outputs)
    TieCall call;
    TieRule t;
    uint32_t which;
};
template <typename T>
hipError_t launch_tie_chunks_t(const TieChunkArgs &a, int64_t grid, hipStream_t st);
template <typename T>
hipError_t launch_tie_gate_t(const pyas_partial *fin, int64_t n, uint32_t which, uint32_t *gate, hipStream_t st);
template <typename T>
hipError_t launch_tie_grid_t(const TieGridArgs &a, hipStream_t st);
template <typename T>
hipError_t launch_tie_pick_t(const pyas_partial *parts, int64_t n, uint32_t which, int64_t base, const TieCall &call,
                             const TieRule &t, uint64_t *keys, hipStream_t st);
template <typename T>
hipError_t launch_tie_finalize_t(const uint64_t *keys, int64_t n_out, int32_t n_sets, const TieCall &call,
                                 const TieRule &t, uint32_t which, pyas_partial *fin, hipStream_t st);
template <typename T>
hipError_t launch_format_t(const pyas_partial *in, int64_t n, int32_t method, void *values,
                           uint8_t *mask, int64_t *counts, hipStream_t st);

// dtype dispatch (pyas_kernels.hip)
hipError_t launch_reduce(int dtype, const ReduceArgs &a, bool shuf, bool bsw, bool masked,
                         int64_t grid, hipStream_t st);
hipError_t launch_finish(int dtype, const FinishArgs &f, hipStream_t st);
hipError_t launch_combine(int dtype, const pyas_partial *in, int64_t n, int64_t seg,
                          int64_t nblocks, uint32_t flags, pyas_partial *out, hipStream_t st);
hipError_t launch_combine_segments(int dtype, const pyas_partial *in, const int64_t *index,
                                   const int64_t *seg, int64_t n_seg, uint32_t flags,
                                   pyas_partial *out, hipStream_t st);
hipError_t launch_reduce_axes(int dtype, const AxesArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_combine_grid(int dtype, const pyas_partial *in, const pyas_grid &g, const CombineTie &ct,
                               int64_t n_out, int64_t n_layers, uint32_t flags,
                               pyas_partial *out, hipStream_t st);
hipError_t launch_axes_dense(int dtype, const AxesArgs &a, bool masked, int64_t grid, hipStream_t st);
hipError_t launch_axes_fold(int dtype, const AxesArgs &a, const FoldGrid &g, bool masked, int64_t grid,
                            hipStream_t st);
hipError_t launch_inflate(const InflateArgs &x, int64_t n, int wbits, hipStream_t st);
hipError_t launch_select(int dtype, const SelectArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_tie_chunks(int dtype, const TieChunkArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_tie_gate(int dtype, const pyas_partial *fin, int64_t n, uint32_t which, uint32_t *gate,
                           hipStream_t st);
hipError_t launch_tie_grid(int dtype, const TieGridArgs &a, hipStream_t st);
hipError_t launch_tie_pick(int dtype, const pyas_partial *parts, int64_t n, uint32_t which, int64_t base,
                           const TieCall &call, const TieRule &t, uint64_t *keys, hipStream_t st);
hipError_t launch_tie_finalize(int dtype, const uint64_t *keys, int64_t n_out, int32_t n_sets, const TieCall &call,
                               const TieRule &t, uint32_t which, pyas_partial *fin, hipStream_t st);
hipError_t launch_format(int dtype, const pyas_partial *in, int64_t n, int32_t method, void *values,
                         uint8_t *mask, int64_t *counts, hipStream_t st);
// second moments (pyas_moments.hip): count / mean / m2 records
struct MomentsArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // workgroups per chunk (full: tiles per chunk)
    const int64_t *out_offsets;       // NULL (full only): chunk c's record at out[c]
    pyas_moments *out;
    pyas_moments *tiles;              // full with bpc > 1: one record per workgroup
    bool bswap, masked;
    bool row;                         // innermost dim reduced: a wave per output
};
hipError_t launch_moments_full(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_moments_axes(int dtype, const MomentsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_moments_tiles(const pyas_moments *tiles, int64_t tpc, int64_t n_chunks,
                                const int64_t *out_offsets, pyas_moments *out, hipStream_t st);
hipError_t launch_moments_segments(const pyas_moments *in, const int64_t *index, const int64_t *seg,
                                   int64_t n_seg, pyas_moments *out, hipStream_t st);
hipError_t launch_moments_grid(const pyas_moments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                               pyas_moments *out, hipStream_t st);
// co-moments of two variables (pyas_comoments.hip): count / means / m2s / cxy records
struct ComomentsArgs {
    ReduceArgs x;                     // x.out unused; the geometry and the selection of both sides
    ReduceArgs y;                     // data, offsets, mask and tab only
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // workgroups per chunk (full: tiles per chunk)
    const int64_t *out_offsets;       // NULL (full only): chunk c's record at out[c]
    pyas_comoments *out;
    pyas_comoments *tiles;            // full with bpc > 1: one record per workgroup
    bool bswap_x, bswap_y, masked_x, masked_y, shuf_x, shuf_y;
    bool row;                         // innermost dim reduced: a wave per output
};
hipError_t launch_comoments_full(int dtype, const ComomentsArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_comoments_axes(int dtype, const ComomentsArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_comoments_tiles(const pyas_comoments *tiles, int64_t tpc, int64_t n_chunks,
                                  const int64_t *out_offsets, pyas_comoments *out, hipStream_t st);
hipError_t launch_comoments_segments(const pyas_comoments *in, const int64_t *index, const int64_t *seg,
                                     int64_t n_seg, pyas_comoments *out, hipStream_t st);
hipError_t launch_comoments_grid(const pyas_comoments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                                 pyas_comoments *out, hipStream_t st);
// least-squares trend against a coordinate (pyas_trend.hip): pyas_comoments records, x = the coordinate
struct TrendArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims (cdim among them)
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;       // NULL (every dim reduced only): chunk c's record at out[c]
    pyas_comoments *out;
    const double *cpool;              // pyas_coord
    const int32_t *corigin;
    int32_t cdim;
    bool shuf, bswap;
    bool row;                         // innermost dim reduced: a wave per output
};
constexpr int kTrendV = 4;            // k_trend_cols: consecutive outputs per lane
constexpr int kTrendRows = 1024;      // k_trend_cols: rows of a chunk layer staged in LDS per pass
struct TrendColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int32_t P;                        // dims 0 .. P-1 are reduced, P .. ndim-1 kept
    int32_t cdim;                     // < P
    const double *cpool;              // pyas_coord
    const int32_t *corigin;
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along the reduced dims / kept dims
    int64_t bpc;                      // workgroups per column
    pyas_comoments *out;              // one finished record per final output
    bool bswap, masked;
};
hipError_t launch_trend_axes(int dtype, const TrendArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_trend_cols(int dtype, const TrendColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_trend_finalize(const pyas_comoments *in, int64_t n, int32_t what, double *value, uint8_t *masked,
                                 hipStream_t st);
// spells past a threshold (pyas_spell.hip): pyas_spell records, merged in sequence order
struct SpellTest {
    double threshold;                 // as the kernel compares: negated for lt / le
    int32_t min_length;
    bool neg, incl;                   // lt / le: compare -x > -threshold; ge / le: equality counts
};
struct SpellArgs {
    ReduceArgs r;                     // r.out unused
    int32_t dim;                      // the one reduced dim
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;       // NULL (1-D variables only): chunk c's record at out[c]
    pyas_spell *out;
    SpellTest t;
    bool shuf, bswap;
    bool row;                         // dim is the innermost dim: a wave per output
};
struct SpellColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along dim 0 / the kept dims
    int64_t bpc;                      // workgroups per column
    pyas_spell *out;                  // one finished record per final output
    SpellTest t;
    bool bswap, masked;
};
hipError_t launch_spell_axes(int dtype, const SpellArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_spell_cols(int dtype, const SpellColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_spell_segments(const pyas_spell *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                 pyas_spell *out, hipStream_t st);
hipError_t launch_spell_grid(const pyas_spell *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                             pyas_spell *out, hipStream_t st);
hipError_t launch_spell_finalize(const pyas_spell *in, int64_t n, int32_t stat, int32_t *value, uint8_t *masked,
                                 hipStream_t st);
// arg-extremes (pyas_argext.hip): pyas_argext records, merged in any order
struct ArgextArgs {
    ReduceArgs r;                     // r.out unused
    int32_t dim;                      // the one reduced dim
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;       // NULL (1-D variables only): chunk c's record at out[c]
    pyas_argext *out;
    const int32_t *origin;            // [n_chunks]: the global index along dim of chunk c's local index 0
    bool neg;                         // argmin
    bool shuf, bswap;
    bool row;                         // dim is the innermost dim: a wave per output
};
struct ArgextColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along dim 0 / the kept dims
    int64_t bpc;                      // workgroups per column
    pyas_argext *out;                 // one finished record per final output
    const int32_t *origin;            // [n_chunks]: the global row of chunk c's row 0
    bool neg;                         // argmin
    bool bswap, masked;
};
hipError_t launch_argext_axes(int dtype, const ArgextArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_argext_cols(int dtype, const ArgextColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
// the combines' launchers for the class of `dtype` and the direction (the merge compares in that class)
typedef hipError_t (*argext_segments_fn)(const pyas_argext *, const int64_t *, const int64_t *, int64_t,
                                         pyas_argext *, hipStream_t);
typedef hipError_t (*argext_grid_fn)(const pyas_argext *, const pyas_grid &, int64_t, int64_t, pyas_argext *,
                                     hipStream_t);
argext_segments_fn launch_argext_segments(int dtype, bool neg);
argext_grid_fn launch_argext_grid(int dtype, bool neg);
hipError_t launch_argext_finalize(const pyas_argext *in, int64_t n, int32_t *index, uint8_t *masked,
                                  hipStream_t st);
// conditional reductions past a threshold (pyas_exceed.hip): pyas_exceed records, merged by addition
struct ExcTest {
    double threshold;                 // the scalar as the kernel compares: negated for lt / le
    bool neg, incl;                   // lt / le: compare -x > -threshold; ge / le: equality counts
    const double *values;             // pyas_exceed_field (NULL: the scalar)
    const int64_t *origin;
    int64_t stride[PYAS_MAX_DIMS];
};
struct ExceedArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // workgroups per chunk (full: tiles per chunk)
    const int64_t *out_offsets;       // NULL (full only): chunk c's record at out[c]
    pyas_exceed *out;
    pyas_exceed *tiles;               // full with bpc > 1: one record per workgroup
    ExcTest t;
    bool bswap, masked;
    bool row;                         // innermost dim reduced: a wave per output
};
struct ExceedColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int32_t P;                        // dims 0 .. P-1 are reduced, P .. ndim-1 kept
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along the reduced dims / kept dims
    int64_t bpc;                      // workgroups per column
    pyas_exceed *out;                 // one finished record per final output
    ExcTest t;
    bool bswap, masked;
};
hipError_t launch_exceed_full(int dtype, const ExceedArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_exceed_axes(int dtype, const ExceedArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_exceed_cols(int dtype, const ExceedColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_exceed_tiles(const pyas_exceed *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                               pyas_exceed *out, hipStream_t st);
hipError_t launch_exceed_segments(const pyas_exceed *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                  pyas_exceed *out, hipStream_t st);
hipError_t launch_exceed_grid(const pyas_exceed *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                              pyas_exceed *out, hipStream_t st);
hipError_t launch_exceed_finalize(const pyas_exceed *in, int64_t n, int32_t stat, const uint8_t *thr_masked,
                                  void *value, uint8_t *masked, hipStream_t st);
// running-window extremes (pyas_rolling.hip): pyas_roll records, merged in sequence order
struct RollArgs {
    ReduceArgs r;                     // r.out unused
    int32_t dim;                      // the one reduced dim
    int32_t window, which;
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;       // NULL (1-D variables only): chunk c's record at out[c]
    pyas_roll *out;
    bool shuf, bswap;
};
struct RollColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along dim 0 / the kept dims
    int64_t bpc;                      // workgroups per column
    pyas_roll *out;                   // one finished record per final output
    int32_t window, which;
    bool bswap, masked;
};
hipError_t launch_roll_axes(int dtype, const RollArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_roll_cols(int dtype, const RollColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_roll_segments(const pyas_roll *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_roll *out, hipStream_t st);
hipError_t launch_roll_grid(const pyas_roll *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                            pyas_roll *out, hipStream_t st);
hipError_t launch_roll_finalize(const pyas_roll *in, int64_t n, int32_t stat, double *value, uint8_t *masked,
                                hipStream_t st);
// per-label second moments (pyas_grouped.hip): pyas_moments records, one per (output, group)
constexpr int kGroupV = 4;            // k_group_cols: consecutive outputs per lane
constexpr int kGroupRows = PYAS_GROUP_ROWS;   // k_group_cols: rows of the sorted list staged in LDS per pass (16 KiB)
struct GroupColsArgs {
    ReduceArgs r;                     // r.out unused; r.sel NULL: whole chunks
    int32_t P;                        // dims 0 .. P-1 are reduced, P .. ndim-1 kept
    int32_t n_groups;
    const int32_t *row_layer;         // pyas_group_rows
    const int32_t *row_off;
    const int32_t *row_label;
    int64_t n_rows;
    int64_t n_coords[PYAS_MAX_DIMS];  // chunk coordinates per dim (chunk n = C-order position)
    int64_t ostride[PYAS_MAX_DIMS];   // final-output element strides (kept dims)
    int64_t n_layers, n_cols;         // chunks along the reduced dims / kept dims
    int64_t bpc;                      // workgroups per column
    int64_t n_out;                    // final outputs per group
    void *out;                        // out[g * n_out + o]: one finished record per (group, final output);
                                      // pyas_moments (k_group_cols) or pyas_partial (k_group_cols_partial)
    bool bswap, masked;
};
struct GroupAxesArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims (gdim among them)
    int64_t bpc;                      // workgroups per chunk
    const int64_t *out_offsets;       // chunk c's records at out[out_offsets[c] + j * n_keep + o]
    void *out;                        // pyas_moments (k_group_axes) or pyas_partial (k_group_axes_partial)
    const int32_t *gstart;            // pyas_group_lists
    const int32_t *gptr;
    const int32_t *gpos;
    int32_t gdim;
    bool shuf, bswap;
    bool row;                         // innermost dim reduced: a wave per record
};
hipError_t launch_group_axes(int dtype, const GroupAxesArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_group_cols(int dtype, const GroupColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
// per-label sum / count / min / max (pyas_grouped.hip): the same walks over pyas_partial records
hipError_t launch_group_axes_partial(int dtype, const GroupAxesArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_group_cols_partial(int dtype, const GroupColsArgs &a, bool shuf, int64_t grid, hipStream_t st);
// weighted sums (pyas_weighted.hip): count / sum w / sum w x records
struct WsumArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // workgroups per chunk (full: tiles per chunk)
    const int64_t *out_offsets;       // NULL (full only): chunk c's record at out[c]
    pyas_wsum *out;
    pyas_wsum *tiles;                 // full with bpc > 1: one record per workgroup
    const double *wpool;              // pyas_weights
    const int32_t *worigin;
    bool bswap, masked;
    bool row;                         // innermost dim reduced: a wave per output
};
hipError_t launch_wsum_full(int dtype, const WsumArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_wsum_axes(int dtype, const WsumArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_wsum_tiles(const pyas_wsum *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                             pyas_wsum *out, hipStream_t st);
hipError_t launch_wsum_segments(const pyas_wsum *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_wsum *out, hipStream_t st);
hipError_t launch_wsum_grid(const pyas_wsum *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                            pyas_wsum *out, hipStream_t st);
// weighted second moments (pyas_wmoments.hip): count / sw / sw2 / means / m2s / cxy records
struct WcomArgs {
    ReduceArgs x;                     // x.out unused; the geometry and the selection of both sides
    ReduceArgs y;                     // two variables: data, offsets, mask and tab only; else zero
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // workgroups per chunk (full: tiles per chunk)
    const int64_t *out_offsets;       // NULL (full only): chunk c's record at out[c]
    pyas_wcomoments *out;
    pyas_wcomoments *tiles;           // full with bpc > 1: one record per workgroup
    const double *wpool;              // pyas_weights
    const int32_t *worigin;
    bool bswap_x, bswap_y, masked_x, masked_y, shuf_x, shuf_y;
    bool row;                         // innermost dim reduced: a wave per output
};
// wcom1: one variable (y unused); wcom2: two variables
hipError_t launch_wcom1_full(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_wcom1_axes(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_wcom2_full(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_wcom2_axes(int dtype, const WcomArgs &a, int64_t grid, hipStream_t st);
hipError_t launch_wcom_tiles(const pyas_wcomoments *tiles, int64_t tpc, int64_t n_chunks, const int64_t *out_offsets,
                             pyas_wcomoments *out, hipStream_t st);
hipError_t launch_wcom_segments(const pyas_wcomoments *in, const int64_t *index, const int64_t *seg, int64_t n_seg,
                                pyas_wcomoments *out, hipStream_t st);
hipError_t launch_wcom_grid(const pyas_wcomoments *in, const pyas_grid &g, int64_t n_out, int64_t n_layers,
                            pyas_wcomoments *out, hipStream_t st);
// binned counts (pyas_hist.hip): int64 table rows of n_bins + 3 slots
constexpr int kHistLdsBins = 2048;    // most bins of the LDS form (k_hist_full) and of LDS-staged edges
constexpr int kHistMaxCopies = 32;    // k_hist_full: most copies of its LDS table (one per lane of an LDS pass)
constexpr int kHistMinCopies = 4;     //              fewest (one per wave)
constexpr int kHistTabBytes = 16384;  //              copies halve until the tables fit this (or reach the fewest)
struct HistArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // k_hist_axes: workgroups per chunk; k_hist_full: tiles per chunk
    int64_t n_pairs;                  // k_hist_full: n_chunks * bpc (chunk, tile) pairs, shared out over the grid
    const int64_t *out_offsets;       // NULL (every dim reduced): row 0
    const int64_t *out_index;         // NULL: the identity
    unsigned long long *table;
    const double *edges;              // pyas_hist
    int32_t n_bins, uniform;
    double lo, scale;
    int32_t shift;                    // k_hist_full: log2 of the LDS table's copies
    int32_t split;                    // k_hist_axes, innermost dim reduced: waves per output
    bool bswap, masked;
    bool row;                         // innermost dim reduced
};
hipError_t launch_hist_full(int dtype, const HistArgs &a, bool shuf, int64_t grid, size_t lds, hipStream_t st);
hipError_t launch_hist_axes(int dtype, const HistArgs &a, bool shuf, int64_t grid, hipStream_t st);
// radix select (pyas_select.hip): one digit's counts per pass, in the histogram's table rows (2^bits + 3 slots)
constexpr int kQselMaxBits = 11;      // 2^11 slots: the most of k_hist_full's LDS tables (kHistLdsBins)
struct QselArgs {
    ReduceArgs r;                     // r.out unused
    uint32_t axes;                    // reduced dims
    int64_t bpc;                      // k_qsel_axes: workgroups per chunk; k_qsel_full: tiles per chunk
    int64_t n_pairs;                  // k_qsel_full: n_chunks * bpc (chunk, tile) pairs, shared out over the grid
    const int64_t *out_offsets;       // NULL (every dim reduced): row 0
    const int64_t *out_index;         // NULL: the identity
    unsigned long long *table;
    const unsigned long long *prefix; // pyas_select: one per table row, NULL on the first pass
    int32_t shift, bits;
    int32_t shift_copies;             // k_qsel_full: log2 of the LDS table's copies
    int32_t split;                    // k_qsel_axes, innermost dim reduced: waves per output
    bool bswap, masked;
    bool row;                         // innermost dim reduced
};
hipError_t launch_qsel_full(int dtype, const QselArgs &a, bool shuf, int64_t grid, size_t lds, hipStream_t st);
hipError_t launch_qsel_axes(int dtype, const QselArgs &a, bool shuf, int64_t grid, hipStream_t st);
hipError_t launch_qsel_step(const unsigned long long *table, int64_t n_rows, int32_t bits, const int64_t *rank,
                            unsigned long long *prefix, const int64_t *below_base, hipStream_t st);
hipError_t launch_qsel_totals(const unsigned long long *table, int64_t n_rows, int32_t bits, int64_t *totals,
                              hipStream_t st);
// host ingest (pyas_ingest.hip): pread ring -> pinned slots -> H2D
struct Ingest;
Ingest *ingest_create(int device);
void ingest_destroy(Ingest *g);
int ingest_configure(Ingest *g, int32_t n_slots, int64_t slot_bytes, std::string &msg);
// zlib_out > 0: every range is a zlib stream inflated on the reader thread
// into exactly zlib_out bytes of its staging slot (status[i] != 0 when it is
// not: a pyas_inflate_status, or PYAS_INFLATE_OVERFLOW for a short output).
int ingest_read(Ingest *g, int fd, int64_t n, const int64_t *file_offsets, const int64_t *sizes,
                uint8_t *dst, const int64_t *dst_offsets, int32_t threads, hipStream_t st,
                std::string &msg, int64_t zlib_out = 0, int32_t *status = nullptr);
// zlib.decompress of one stream (RFC 1950) into at most `cap` bytes of dst;
// a pyas_inflate_status, n_out = bytes written (pyas_ingest.hip).
int host_inflate(const uint8_t *src, int64_t n_src, uint8_t *dst, int64_t cap, int64_t &n_out);

// pyas_capi.hip: the thread-local pyas_last_error() message, and the device a
// context is bound to (for runtime pieces in other translation units)
int set_error(int code, const char *fmt, ...);
int ctx_device(const pyas_ctx *ctx);

hipError_t launch_unshuffle_chunks(const void *src, const int64_t *soff, void *dst, const int64_t *doff,
                                   int64_t n_chunks, int64_t nbytes, int64_t es, hipStream_t st);
hipError_t launch_unshuffle(const void *src, void *dst, int64_t nbytes, int64_t es,
                            hipStream_t st);

}  // namespace pyas
