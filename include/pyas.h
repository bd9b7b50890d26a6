/*
 * pyas.h — C ABI of the MI355X (gfx950) chunk-reduction backend.
 *
 * Drop-in boundary for PyActiveStorage's local chunk reducer.  Every entry
 * point below names the reference interface it replaces (paths relative to
 * the NCAS-CMS/PyActiveStorage repository):
 *
 *   reference                                       | replaced by
 *   ------------------------------------------------+---------------------------
 *   activestorage/storage.py:8-104  reduce_chunk    | pyas_reduce_chunks (batch,
 *     (one call per chunk, NumPy)                   |   method != None)
 *   activestorage/storage.py:95-96  chunk[sel] +    | pyas_select_chunks
 *     mask_missing  (method=None branch, :102-103)  |
 *   activestorage/storage.py:98-100 np.ma.count +   | pyas_reduce_axes (partial
 *     method(axis=..., keepdims=True), axis ⊂ dims  |   axis reductions)
 *   activestorage/storage.py:107-123 filter_pipeline| fused into the kernels
 *     + numcodecs.Shuffle.decode (hdf2numcodec:37)  |   (pyas_batch.shuffle) and
 *                                                   |   pyas_unshuffle
 *   activestorage/storage.py:119-120 compression.   | pyas_inflate (zlib streams,
 *     decode = numcodecs.Zlib (hdf2numcodec:34-35)  |   one wave per chunk)
 *   activestorage/storage.py:126-153 mask_missing   | pyas_mask (thresholds are
 *                                                   |   pre-compiled on the host)
 *   activestorage/storage.py:51-53,156-162 open +   | pyas_read_ranges (pread
 *     read_block, once per chunk                    |   ring -> pinned -> H2D)
 *   activestorage/active.py:557-598 thread-pool     | pyas_reduce_chunks with a
 *     fan-out + out[...] assembly + method(out)     |   `total` output, and
 *                                                   |   pyas_combine_partials
 *
 * Conventions
 *   - Plain C types only; every pointer documented as "device" must be a HIP
 *     device (or managed) pointer on the context's device.  `stream` is a
 *     hipStream_t passed as void* (NULL = the null stream).
 *   - Every function returns a pyas_status; on failure pyas_last_error()
 *     returns a thread-local message.  Launch functions do not synchronise
 *     and allocate nothing after the first call with a given geometry, so a
 *     caller may capture them into a hipGraph after one warm call.
 *   - Results are deterministic: no floating-point atomics anywhere; partials
 *     are combined in a fixed order.
 */
#ifndef PYAS_H
#define PYAS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYAS_ABI_VERSION 2
#define PYAS_MAX_DIMS 8

typedef enum {
    PYAS_OK = 0,
    PYAS_EINVAL = 1,      /* bad argument (reference: ValueError)            */
    PYAS_ENOTSUP = 2,     /* unsupported dtype/filter (NotImplementedError)  */
    PYAS_EDEVICE = 3,     /* HIP runtime / launch failure                    */
    PYAS_ENOMEM = 4,      /* device allocation failed                        */
    PYAS_EINDEX = 5,      /* selection out of the chunk (IndexError)         */
    PYAS_EIO = 6          /* file read failed or ended early (OSError)       */
} pyas_status;

/* netCDF-4 numeric types (the 10 the format defines) */
typedef enum {
    PYAS_I8 = 0, PYAS_U8 = 1, PYAS_I16 = 2, PYAS_U16 = 3, PYAS_I32 = 4,
    PYAS_U32 = 5, PYAS_I64 = 6, PYAS_U64 = 7, PYAS_F32 = 8, PYAS_F64 = 9
} pyas_dtype;

/* One 8-byte value in the data's class: f for floats, i for signed, u for
 * unsigned integers.  Float data values (f32 too) are carried exactly as f64. */
typedef union {
    double f;
    int64_t i;
    uint64_t u;
} pyas_scalar;

/* Partial result of a masked reduction over a set of elements (32 bytes).
 * sum  : floats accumulate in f64; signed ints in int64, unsigned in uint64,
 *        both wrapping modulo 2^64 exactly as NumPy's int64/uint64 sums do.
 * count: unmasked elements (np.ma.count, storage.py:98).
 * min/max: NaN-propagating like np.ma.min/max; meaningless when count == 0
 *        (the reference returns `masked` there, storage.py:99-100). */
typedef struct {
    pyas_scalar sum;
    int64_t count;
    pyas_scalar min;
    pyas_scalar max;
} pyas_partial;

/* Compiled form of mask_missing (storage.py:126-153).  All thresholds are
 * values OF THE DATA TYPE (already converted by the host so that the device
 * comparison in the data type is exactly NumPy's comparison in the promoted
 * type).  An element x is masked iff
 *     (eq_lo[0] <= x <= eq_hi[0]) || (eq_lo[1] <= x <= eq_hi[1])
 *  || x > gt || x < lt  || (vector tables, below).
 * Disabled rules use neutral values (empty interval lo > hi; gt = +inf or
 * type max; lt = -inf or type min) and their bit is clear in `flags`.
 * Vector _FillValue / missing_value (storage.py:133-143, broadcast equality)
 * use device tables of intervals indexed by sum_d idx_d * tab_stride[k][d],
 * idx_d = position inside the chunk's selection along chunk dim d. */
#define PYAS_MASK_EQ0 1u
#define PYAS_MASK_EQ1 2u
#define PYAS_MASK_GT 4u
#define PYAS_MASK_LT 8u
#define PYAS_MASK_TAB0 16u
#define PYAS_MASK_TAB1 32u

typedef struct {
    uint32_t flags;
    int32_t tab_len[2];
    pyas_scalar eq_lo[2];
    pyas_scalar eq_hi[2];
    pyas_scalar gt;
    pyas_scalar lt;
    const pyas_scalar *tab_lo[2];           /* device, tab_len[k] entries */
    const pyas_scalar *tab_hi[2];
    int64_t tab_stride[2][PYAS_MAX_DIMS];
} pyas_mask;

/* A batch of chunks of ONE variable resident in device memory.
 * Chunk c occupies bytes [offsets[c], offsets[c] + chunk_nbytes) of `data`
 * (uncompressed; byte-shuffled when `shuffle` > 1; big-endian when
 * `byteswap`).  offsets[c] must be a multiple of the element size.
 * Selection (storage.py:95 chunk[chunk_selection]) per chunk and chunk dim:
 *   sel[(c*PYAS_MAX_DIMS + d)*3 + {0,1,2}] = {start, step, count}
 *   step != 0 : indices start + k*step, k < count   (slices; step may be < 0)
 *   step == 0 : indices index_pool[start + k], k < count (integer lists)
 * sel == NULL selects every chunk completely. */
typedef struct {
    int32_t dtype;                     /* pyas_dtype */
    int32_t byteswap;                  /* 1: stored non-native (big-endian) */
    int32_t shuffle;                   /* HDF5 shuffle element size, 0/1 = off */
    int32_t ndim;                      /* chunk rank, 1..PYAS_MAX_DIMS */
    int64_t chunk_shape[PYAS_MAX_DIMS];
    int64_t n_chunks;
    const void *data;                  /* device */
    const int64_t *offsets;            /* device [n_chunks] */
    const int32_t *sel;                /* device [n_chunks*PYAS_MAX_DIMS*3] or NULL */
    const int32_t *index_pool;         /* device, used by step == 0 dims */
} pyas_batch;

/* combine flags */
#define PYAS_COMBINE_ROUND_TO_VAR 1u   /* round each input sum to the variable
                                          dtype first (Active stores partials in
                                          an `out` array of the var dtype,
                                          active.py:512,585) */

typedef struct pyas_ctx pyas_ctx;

/* ---- library / context -------------------------------------------------- */
int pyas_abi_version(void);
const char *pyas_last_error(void);
int pyas_device_count(int *count);
int pyas_ctx_create(int device, pyas_ctx **out);
int pyas_ctx_destroy(pyas_ctx *ctx);
/* Tile size (bytes of selected data per workgroup); 0 restores the default. */
int pyas_ctx_set_tile_bytes(pyas_ctx *ctx, int64_t tile_bytes);
/* LDS history ring of pyas_inflate, 2^wbits bytes per stream, wbits in
 * [13, 15] (default 13).  Smaller rings run more streams per CU; matches
 * reaching past the ring read the already-written output.  Results do not
 * depend on it. */
int pyas_ctx_set_inflate_window_bits(pyas_ctx *ctx, int32_t wbits);
/* on != 0 (default): pyas_reduce_chunks folds tiles -> chunks -> groups ->
 * total in one finishing launch (the last group to finish folds the total,
 * in group order); 0: the total is folded by a second launch.  Results are
 * bit-identical either way. */
int pyas_ctx_set_chained_combine(pyas_ctx *ctx, int32_t on);
/* pyas_reduce_axes_grid launches n_cols x (workgroups per column); it splits
 * the reduced rows further until the launch has >= n workgroups, and refuses
 * (PYAS_ENOTSUP, two-step path) below n / 4.  0 restores the default 2048. */
int pyas_ctx_set_fold_min_blocks(pyas_ctx *ctx, int64_t n);

/* ---- NumPy's sign of a zero min/max -------------------------------------
 * storage.py:99-100 returns np.ma.min/max(chunk[sel], axis, keepdims=True),
 * and active.py:594 reduces the `out` array of per-chunk results the same
 * way.  When an extreme is zero and +0.0 and -0.0 both occur, the zero NumPy
 * returns is decided by the order its reduction visits the elements
 * (pyactivestorage_amd/zerosign.py states the measured rules): the iterator
 * walks the reduced array in memory order; every run of the trailing
 * reduced dims is one call of the reduce loop, cut into pieces of
 * np.getbufsize() elements; a contiguous call keeps one accumulator per SIMD
 * lane seeded with the running result (later wins in a lane, lanes folded
 * in a fixed priority, then a scalar remainder); a strided call keeps `acc`
 * accumulators seeded with its first elements; an elementwise loop (kept
 * innermost dim) lets every later zero win.  The lane counts and priorities
 * depend on the SIMD target NumPy dispatches on the host, so the host derives
 * them from NumPy and sets them per float dtype:
 *   lanes 1..64, piece 1..2^24, rank[lane] = priority (0 wins every tie),
 *   acc 1..64 accumulators of the strided loop, acc_rank likewise. */
typedef struct {
    int32_t lanes;
    int32_t piece;
    int32_t acc;
    uint8_t rank[64];
    uint8_t acc_rank[64];
} pyas_tie_rule;
/* dtype PYAS_F32 or PYAS_F64; rule NULL clears it (no sign rewriting). */
int pyas_ctx_set_tie_rule(pyas_ctx *ctx, int32_t dtype, const pyas_tie_rule *rule);

/* How NumPy walks chunk[sel] (after mask_missing) for one query:
 * perm = chunk dims (the batch's dim order) from outer to inner in memory;
 * PYAS_TIE_VIEW: the array is the chunk[sel] view itself (no mask attribute
 * and slices only), so its strides are step * chunk stride; otherwise it is
 * a copy, contiguous in perm order; PYAS_TIE_BUFFERED: non-native byte
 * order (NumPy reduces through a contiguous buffer). */
#define PYAS_TIE_VIEW 1u
#define PYAS_TIE_BUFFERED 2u
typedef struct {
    int32_t perm[PYAS_MAX_DIMS];
    uint32_t flags;
} pyas_tie_geom;

/* Level 1, per chunk (storage.py:99-100): for every output of every chunk of
 * `batch` (the chunk's selection reduced over the dims in axes_mask; outputs
 * row-major over the kept selected dims, at partials[out_offsets[c] + o], or
 * partials[c] when out_offsets is NULL) whose partial has count > 0 and a
 * zero min (which bit 0) / max (bit 1): rewrite that zero's sign as NumPy's
 * (masked elements never tie).  Float dtypes only; a no-op without a rule. */
int pyas_tie_chunks(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_tie_geom *geom, uint32_t axes_mask, uint32_t which,
                    const int64_t *out_offsets, pyas_partial *partials, void *stream);
/* Level 1 of a FULL reduction (every dim reduced, one partial per chunk, the
 * chunks at positions layer_base + c of the `out` array's call of length lr,
 * active.py:594), done only where it can matter: which zero the level-2 keys
 * pick depends on positions alone, so a pick pass keys the zero partials
 * with sign 0, and only the chunk holding the K1 winner and the chunk
 * holding the W winner are scanned (pyas_tie_chunks' scan, one wave each).
 * pyas_tie_segments over the same partials then gives the same result as
 * after pyas_tie_chunks over every chunk (a group of ranks: each rank's keys
 * name its own two chunks, and the exchange picks among them).  Replaces
 * pyas_tie_chunks for storage.py:99-100 + active.py:594 full reductions. */
int pyas_tie_chunks_total(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                          const pyas_tie_geom *geom, uint32_t which, pyas_partial *partials,
                          int64_t layer_base, int64_t lr, void *stream);
/* Level 1 for a result folded without per-chunk partials
 * (pyas_reduce_axes_grid): when any of the n_final partials in `final_`
 * has a zero min/max (which: 1 or 2), write one byte per chunk output to
 * flags[out_offsets[c] + o] (bit 0: the output holds an unmasked zero, bit
 * 1: the sign NumPy's reduction of it returns); otherwise write nothing. */
int pyas_tie_chunk_flags(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                         const pyas_tie_geom *geom, uint32_t axes_mask, uint32_t which,
                         const int64_t *out_offsets, const pyas_partial *final_, int64_t n_final,
                         uint8_t *flags, void *stream);
/* ---- memory helpers (so a non-torch host can drive the ABI) ------------- */
int pyas_malloc(pyas_ctx *ctx, size_t nbytes, void **dptr);
int pyas_free(pyas_ctx *ctx, void *dptr);
/* Pinned (page-locked) host memory: H2D copies from it are DMA, without the
 * runtime's pageable staging.  The per-chunk drop-in reads each chunk
 * (storage.py:51-53 read_block) straight into a per-thread pinned buffer. */
int pyas_host_alloc(pyas_ctx *ctx, size_t nbytes, void **hptr);
int pyas_host_free(pyas_ctx *ctx, void *hptr);
int pyas_memcpy_h2d(pyas_ctx *ctx, void *dst, const void *src, size_t n, void *stream);
int pyas_memcpy_d2h(pyas_ctx *ctx, void *dst, const void *src, size_t n, void *stream);
int pyas_stream_create(pyas_ctx *ctx, void **stream);
int pyas_stream_destroy(pyas_ctx *ctx, void *stream);
int pyas_stream_synchronize(pyas_ctx *ctx, void *stream);
/* Work queued on `waiter` after this call starts only once everything queued
 * on `waitee` so far has finished (an event recorded on waitee, waited on by
 * waiter; no host synchronisation).  Lets ingest copies on one stream
 * overlap device inflate on another (Active's compressed-chunk pipeline). */
int pyas_stream_wait(pyas_ctx *ctx, void *waiter, void *waitee);

/* ---- hot path ------------------------------------------------------------ */
/* Fused un-shuffle -> byte-swap -> select -> mask -> sum/count/min/max for
 * every chunk of the batch.  chunk_out (device, n_chunks entries, may be
 * NULL) receives one partial per chunk (storage.py:98-100 with axis = all
 * dims); total (device, 1 entry, may be NULL) receives the combine of all
 * chunk partials under `combine_flags` (active.py:594-598). */
int pyas_reduce_chunks(pyas_ctx *ctx, const pyas_batch *batch,
                       const pyas_mask *mask, pyas_partial *chunk_out,
                       pyas_partial *total, uint32_t combine_flags,
                       void *stream);

/* Partial-axis reduction: for chunk c the selected block is reduced over the
 * chunk dims whose bit is set in axes_mask; outputs (row-major over the
 * remaining selected dims, keepdims) start at out[out_offsets[c]]. */
int pyas_reduce_axes(pyas_ctx *ctx, const pyas_batch *batch,
                     const pyas_mask *mask, uint32_t axes_mask,
                     const int64_t *out_offsets, pyas_partial *out,
                     void *stream);

/* Compact per-output records (pyas_reduce_axes_ex): what storage.py:98-100
 * returns per chunk for ONE method, with the sum rounded to the variable
 * dtype as Active stores it in its `out` array (active.py:512,585).  A
 * record is a value in the variable dtype -- the sum (PYAS_REC_SUM, for sum
 * and mean; an integer sum wraps to the variable dtype), the min
 * (PYAS_REC_MIN) or the max (PYAS_REC_MAX) -- and an int32 count:
 * PYAS_REC_BYTES(itemsize) bytes, 8 for 1/2/4-byte dtypes (value in the low
 * bytes of the first 4, count in the next 4), 16 for 8-byte dtypes (value,
 * count, 4 zero bytes).  An all-zero record is neutral (count 0).  The
 * combines read them with PYAS_COMBINE_REC(rec) in combine_flags, the
 * zero-sign passes with PYAS_TIE_REC in `which`; their results are
 * bit-identical to the 32-byte path with PYAS_COMBINE_ROUND_TO_VAR. */
#define PYAS_REC_FULL 0    /* the 32-byte pyas_partial */
#define PYAS_REC_SUM 1
#define PYAS_REC_MIN 2
#define PYAS_REC_MAX 3
#define PYAS_REC_BYTES(itemsize) ((itemsize) <= 4 ? 8 : 16)
#define PYAS_COMBINE_REC(rec) ((uint32_t)(rec) << 4)
#define PYAS_TIE_REC 4u    /* which: parts are PYAS_REC_MIN (which 1) / _MAX (which 2) records */
/* OR'ed into pyas_reduce_axes_ex's rec (PYAS_REC_MIN / PYAS_REC_MAX of a
 * float variable): the per-chunk walk writes NumPy's sign of a zero min/max
 * itself (storage.py:99-100), so pyas_tie_chunks need not run.  Column
 * layout (innermost chunk dim kept): the calls are elementwise and the last
 * zero wins.  LDS row layout (innermost dim reduced, rows <= 64 elements, the
 * reduced group that dim alone when chunks are cut): each row is one
 * contiguous call, keyed with the context's tie rule
 * (pyas_ctx_set_tie_rule).  The caller promises every chunk is whole or a unit-step box
 * covering at least half the chunk with more than one index in the
 * innermost dim; PYAS_ENOTSUP when the launch cannot key the sign (another
 * layout, no tie rule, cut chunks it would not take). */
#define PYAS_REC_ZERO_SIGN 0x100
/* OR'ed into pyas_reduce_axes_ex's rec: the caller promises what
 * PYAS_REC_ZERO_SIGN's caller promises (every chunk whole or a unit-step box
 * covering at least half the chunk with more than one index in the innermost
 * dim), so the generic per-element walk is not launched for the chunks the
 * dense launch leaves (there are none).  A broken promise leaves those
 * chunks' outputs unwritten. */
#define PYAS_REC_DENSE_ONLY 0x200
/* The opposite promise: no chunk is whole or such a box (e.g. a strided or
 * listed selection in every chunk), so the dense launch, which would find no
 * chunk of its own, is not made.  A broken promise leaves the whole and box
 * chunks' outputs unwritten. */
#define PYAS_REC_GENERIC_ONLY 0x400
/* pyas_reduce_axes writing `rec` records (PYAS_REC_*; PYAS_REC_FULL is
 * pyas_reduce_axes itself): out[out_offsets[c] + o] in record units.  A
 * chunk's outputs must count < 2^31 elements each. */
int pyas_reduce_axes_ex(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                        uint32_t axes_mask, int32_t rec, const int64_t *out_offsets, void *out,
                        void *stream);

/* method=None: decode + select + mask into dense row-major outputs.
 * values (device) receives native-endian elements, mask_out (device, may be
 * NULL) one byte per element (1 = masked); chunk c starts at element
 * out_offsets[c]. */
int pyas_select_chunks(pyas_ctx *ctx, const pyas_batch *batch,
                       const pyas_mask *mask, const int64_t *out_offsets,
                       void *values, uint8_t *mask_out, void *stream);

/* method=None for a whole orthogonal query (Active._select, active.py:
 * 483-485 -> storage.py:95-103 per chunk, then the reference places each
 * chunk's selection at its out_selection): element k = (k_0..k_{n-1}) of
 * chunk c's selection (C order over the selection counts) is written to
 * values/mask_out at  sum_d pos[chunk_base[c*ndim + d] + k_d] * out_stride[d]
 * (an element index of the caller's output array).  pos (int64) and
 * chunk_base (int32) are device arrays; dims dropped by an integer index use
 * out_stride 0. */
typedef struct {
    const int64_t *pos;
    const int32_t *chunk_base;
    int64_t out_stride[PYAS_MAX_DIMS];
} pyas_scatter;

int pyas_select_scatter(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                        const pyas_scatter *scatter, void *values, uint8_t *mask_out,
                        void *stream);

/* Fixed-order combine of n partials (device) into *out (device).  Used for
 * the per-chunk -> total step and for the cross-GPU combine of per-rank
 * partials after an RCCL all-gather. */
int pyas_combine_partials(pyas_ctx *ctx, int32_t dtype, const pyas_partial *in,
                          int64_t n, uint32_t combine_flags, pyas_partial *out,
                          void *stream);

/* ---- several GPUs in one process (active.py:557-598 across devices) ------
 * Each of the ndev contexts (distinct devices) reduces its own batch of the
 * SAME variable on its own stream (pyas_reduce_chunks, combine_flags as
 * there); the per-device totals then travel in ONE RCCL all-gather over
 * xGMI (communicators over the listed devices, created with
 * ncclCommInitAll on first use of a device list and kept until
 * pyas_shard_release) and every device folds them in list order.
 * out[k] (device memory of ctx[k], ndev + 1 partials): out[k][0] receives
 * the global total, identical on every device; out[k][1 + j] the total of
 * device j.  mask may be NULL (unmasked) or hold one mask per device.
 * Asynchronous like every launch: synchronise streams[k] before reading.
 * Bounded wait: with the environment variable PYAS_SHARD_TIMEOUT_MS set to
 * a number >= 0 the call instead waits for the exchange up to that many
 * milliseconds (0: one poll), polling the streams and ncclCommGetAsyncError.
 * On an RCCL or stream error, or on expiry once every device has reached
 * its collectives (a stalled peer), it aborts the device list's
 * communicators (ncclCommAbort), drops them from the cache and returns
 * PYAS_EDEVICE naming the devices that had not finished; the streams and
 * out buffers of that call are then to be discarded.  On expiry while a
 * device is still reducing (its collectives queued, not started) it keeps
 * the communicators -- aborting would free them under queued RCCL kernels
 * -- and returns PYAS_EDEVICE naming the busy devices; the exchange then
 * completes on the streams.  Verified on hardware at ndev = 1.
 * Thread safety: calls on the same device list are serialised from group
 * start to group end (RCCL allows one group on a communicator at a time);
 * pyas_shard_release waits for a call still using a set.
 * Zero sign: this entry returns the combined partial as the devices reduce
 * it; pyas_reduce_sharded_tie below applies storage.py/active.py's
 * +0.0/-0.0 rule (as pyactivestorage_amd.distributed does).
 * RCCL is resolved from the process first (an RCCL already mapped, e.g.
 * torch's), then librccl.so.1.
 * The multi-process equivalent (one process per GPU) is
 * pyactivestorage_amd.distributed over torch.distributed. */
int pyas_reduce_sharded(pyas_ctx *const *ctx, const pyas_batch *const *per_dev,
                        const pyas_mask *const *mask, int32_t ndev, uint32_t combine_flags,
                        pyas_partial *const *out, void *const *streams);
/* pyas_reduce_sharded with NumPy's sign of a zero min (which = 1) or max
 * (which = 2) of a float variable (storage.py:99-100 per chunk, active.py:594
 * over the per-chunk results): device k's chunks are positions
 * [sum of earlier devices' n_chunks, + n_chunks) of the query's chunk order
 * (the `out` array); each device keeps its per-chunk partials (per-call
 * scratch), keys its two candidate chunks (pyas_tie_chunks_total) and its
 * total (pyas_tie_segments), the 16-byte keys travel in the same RCCL group
 * as the totals, and every device applies pyas_tie_finalize to out[k][0].
 * The tie rule of the dtype must be set on every ctx
 * (pyas_ctx_set_tie_rule); without one, and for integer dtypes or which = 0,
 * this is pyas_reduce_sharded.  `geom` as for pyas_tie_chunks. */
int pyas_reduce_sharded_tie(pyas_ctx *const *ctx, const pyas_batch *const *per_dev,
                            const pyas_mask *const *mask, int32_t ndev, uint32_t combine_flags,
                            const pyas_tie_geom *geom, uint32_t which,
                            pyas_partial *const *out, void *const *streams);
/* Destroy the cached RCCL communicators of pyas_reduce_sharded (waits for a
 * call still using them). */
int pyas_shard_release(void);

/* Segmented fixed-order combine: out[s] = fold of in[index[k]] for k in
 * [seg_offsets[s], seg_offsets[s+1]) in order (device arrays).  This is the
 * partial-axis form of the Active combine (active.py:575-598): `in` holds
 * per-chunk partial arrays, each segment lists the partials that fall on one
 * output element along the reduced axes. */
int pyas_combine_segments(pyas_ctx *ctx, int32_t dtype, const pyas_partial *in,
                          const int64_t *index, const int64_t *seg_offsets,
                          int64_t n_segments, uint32_t combine_flags,
                          pyas_partial *out, void *stream);

/* Box-query form of the partial-axis combine (active.py:487-516,591-598:
 * each chunk's partial array is placed at its out_selection in `out`, then
 * method(out, axis) folds the chunk layers).  For an orthogonal selection the
 * chunks are the C-ordered product of per-dim chunk-coordinate lists, so the
 * segments of pyas_combine_segments follow from small per-dim tables and no
 * per-output index list is built on the host.  Output element f (C order
 * over out_extent) folds, in C order over the reduced dims' coordinates,
 * in[chunk_out_offsets[n] + j] where n is the chunk's position in the
 * product and j the element's index in that chunk's kept-dims partial array
 * (C order over the chunk's selected counts, reduced dims of extent 1). */
typedef struct {
    int32_t ndim;
    uint32_t axes_mask;                          /* reduced dims */
    int64_t n_coords[PYAS_MAX_DIMS];             /* chunk coordinates per dim */
    int64_t out_extent[PYAS_MAX_DIMS];           /* kept dims: final extent; reduced: 1 */
    const int32_t *pos_coord[PYAS_MAX_DIMS];     /* kept dims (device): position -> coordinate index */
    const int32_t *pos_local[PYAS_MAX_DIMS];     /* kept dims (device): position -> index in that chunk's selection */
    const int32_t *coord_count[PYAS_MAX_DIMS];   /* kept dims (device): coordinate index -> selected count */
    const int64_t *chunk_out_offsets;            /* device [prod n_coords] (pyas_reduce_axes's out_offsets) */
} pyas_grid;

int pyas_combine_grid(pyas_ctx *ctx, int32_t dtype, const pyas_partial *in,
                      const pyas_grid *grid, uint32_t combine_flags, pyas_partial *out,
                      void *stream);

/* pyas_reduce_axes + pyas_combine_grid in ONE launch, for a box query whose
 * chunks are all whole (batch->sel == NULL) and laid out in the grid's C
 * order (chunk n = grid position n, prod n_coords chunks), each kept dim's
 * final extent being n_coords x the chunk extent.  The chunk layers along the
 * reduced dims are folded inside the reduction kernel, in the same order and
 * with the same rounding as pyas_combine_grid, so `out` (device, one partial
 * per final element) is bit-identical to the two-step result while the
 * per-chunk partial arrays are never written.  Only grid->ndim, axes_mask,
 * n_coords and out_extent are read.  Returns PYAS_ENOTSUP (nothing launched)
 * when the geometry does not admit it (element size < 4 bytes, shuffled
 * bytes, vector mask tables, or a reduced innermost dim): the caller then
 * takes the two-step path. */
int pyas_reduce_axes_grid(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                          const pyas_grid *grid, uint32_t combine_flags, pyas_partial *out,
                          void *stream);
/* combine_flags of pyas_reduce_axes_grid: NumPy's sign of a zero min (MIN)
 * or max (MAX), fused into the fold, so pyas_tie_chunk_flags and
 * pyas_tie_grid are not needed.  The caller checks that the chunks are
 * C-ordered (NumPy reduces chunk[sel] in memory order, storage.py:99-100);
 * the library derives both NumPy calls from the geometry:
 *  - lean column fold (innermost dim kept): valid where both reductions are
 *    elementwise (the chunks' innermost non-1 dim and the `out` array's,
 *    active.py:594, are kept) -- every later zero wins, and each lane tracks
 *    its outputs' last zero (layer order, then row order);
 *  - LDS row fold (modes 4-6, each output row one contiguous call): the
 *    context's tie rule (pyas_ctx_set_tie_rule) keys the zeros of a row
 *    whose min/max is a zero, and the row's sign is keyed at its layer's
 *    position in the `out` array's call (MIN or MAX, not both).
 * Float dtypes; PYAS_ENOTSUP (nothing launched) when the geometry takes
 * another fold kernel, a reduction the kernel cannot key, or no rule is set:
 * fold without the flag and run the zero-sign passes then.
 * pyas_combine_grid takes the same flags over records that already carry
 * level 1's signs (pyas_reduce_axes_ex with PYAS_REC_ZERO_SIGN) and keys
 * level 2 itself, so pyas_tie_grid is not needed: where the `out` array's
 * calls are elementwise (its innermost non-1 dim kept) each output takes the
 * sign of its last layer whose min (max) is a zero; where they run over the
 * trailing reduced dims (calls of lr layers), the context's tie rule keys the
 * zero layers at their positions in the call (pyas_tie_grid's keys). */
#define PYAS_FOLD_ZERO_SIGN_MIN 0x100u
#define PYAS_FOLD_ZERO_SIGN_MAX 0x200u

/* ---- NumPy's sign of a zero min/max, level 2 (see pyas_tie_chunks) ---- */
/* Level 2, across chunks (active.py:594): every final output f (partials
 * final_, device) whose min (which 1) / max (which 2) is a zero gets the sign
 * NumPy's reduction of the `out` array returns.  The chunk layers of f are
 * walked as pyas_combine_grid walks them; layer l's value comes from the
 * level-1 partials (`parts`, pyas_reduce_axes layout) or flag bytes
 * (`flags`).  lr: the length of one reduce call over `out` (the product of
 * its trailing reduced extents, 1 when its innermost non-1 dim is kept).
 * keys NULL: the sign is written to final_; else K1 keys are folded into
 * keys[f] (max) and W keys into keys[n_out + f] (min), for ranks of a group
 * to combine with pyas_tie_finalize (keys set up by pyas_tie_keys_reset). */
int pyas_tie_grid(pyas_ctx *ctx, int32_t dtype, const pyas_grid *grid, const pyas_partial *parts,
                  const uint8_t *flags, int64_t lr, uint32_t which, pyas_partial *final_,
                  uint64_t *keys, void *stream);
/* Level 2 over segments (pyas_combine_segments' layout: layer k of output s
 * is parts[index[seg[s] + k]]), or, with index == seg == NULL, one output
 * whose layers are parts[0 .. n_layers) (a full reduction; n_seg == 1).
 * Layer k sits at reduced position layer_base + k (a rank's first chunk). */
int pyas_tie_segments(pyas_ctx *ctx, int32_t dtype, const pyas_partial *parts, const int64_t *index,
                      const int64_t *seg, int64_t n_seg, int64_t n_layers, int64_t layer_base,
                      int64_t lr, uint32_t which, pyas_partial *final_, uint64_t *keys, void *stream);
/* keys (device, 2 * n_out): K1 = 0, W = all ones. */
int pyas_tie_keys_reset(pyas_ctx *ctx, uint64_t *keys, int64_t n_out, void *stream);
/* Combine n_sets key arrays (device, n_sets x [K1[n_out], W[n_out]]) and
 * write the signs into final_'s zero min/max. */
int pyas_tie_finalize(pyas_ctx *ctx, int32_t dtype, const uint64_t *keys, int64_t n_out, int32_t n_sets,
                      int64_t lr, uint32_t which, pyas_partial *final_, void *stream);

/* ---- second moments (Active.var / Active.std) ------------------------------
 * Partial record of a masked variance over a set of elements (32 bytes):
 * count unmasked elements; mean of them; m2 = sum (x - mean)^2  (all in f64).
 * count == 0 is neutral (mean, m2 ignored; written as 0).  Integer values
 * convert to f64 as astype(float64) does.  One pass: each lane keeps a shift K
 * (its first unmasked value) with sum (x-K) and sum (x-K)^2 in f64; lanes,
 * waves, tiles and chunks merge in a fixed order with Chan's formula
 *   d = mean_b - mean_a;  mean = mean_a + d n_b/n;  m2 = m2_a + m2_b + d^2 n_a n_b/n
 * (a side with count 0 is skipped), so results are bit-identical from run to
 * run.  An unmasked NaN gives NaN mean and m2, an unmasked +-inf a NaN m2.
 * The mean travels as one f64, so a merge of records whose means differ by
 * about sigma costs about 2^-53 |mean| / sigma relative in m2. */
typedef struct { int64_t count; double mean; double m2; uint64_t reserved; } pyas_moments;

/* pyas_reduce_axes for moments: out[out_offsets[c] + o] receives the record
 * of output o (C order over the kept selected dims) of chunk c.  With every
 * dim in axes_mask each chunk yields one record (at out[out_offsets[c]], or
 * out[c] when out_offsets is NULL), streamed with 16-byte loads where the
 * chunk is whole or its selection one contiguous run.  Like pyas_reduce_axes
 * the selection table is trusted (the host checks it: PYAS_EINDEX). */
int pyas_moments_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                      uint32_t axes_mask, const int64_t *out_offsets, pyas_moments *out,
                      void *stream);
/* pyas_combine_segments for moments records (same order: index order inside
 * a segment); index NULL: the identity (segment s folds in[seg[s] .. seg[s+1])). */
int pyas_moments_combine_segments(pyas_ctx *ctx, const pyas_moments *in, const int64_t *index,
                                  const int64_t *seg_offsets, int64_t n_segments,
                                  pyas_moments *out, void *stream);
/* pyas_combine_grid for moments records (same order: C order over the reduced
 * dims' chunk coordinates). */
int pyas_moments_combine_grid(pyas_ctx *ctx, const pyas_moments *in, const pyas_grid *grid,
                              pyas_moments *out, void *stream);

/* ---- co-moments of two variables (Active.cov / Active.corr) -------------------
 * Partial record of a masked covariance over a set of pairs (48 bytes):
 * count pairs unmasked on both sides; mean_x, mean_y of them;
 * m2_x = sum (x - mean_x)^2, m2_y = sum (y - mean_y)^2 and
 * cxy = sum (x - mean_x)(y - mean_y)  (all in f64).  count == 0 is neutral
 * (the other fields ignored; written as 0).  Values convert to f64 as
 * astype(float64) does.  One pass: each lane keeps shifts Kx, Ky (its first
 * counted pair) with sum (x-Kx), sum (y-Ky), sum (x-Kx)^2, sum (y-Ky)^2 and
 * sum (x-Kx)(y-Ky) in f64 (FMA); lanes, waves, tiles and chunks merge in the
 * fixed order of the moments records with
 *   d_x = mean_x_b - mean_x_a;  d_y = mean_y_b - mean_y_a;
 *   cxy = cxy_a + cxy_b + d_x d_y n_a n_b/n
 * and the means and m2s exactly as pyas_moments merges them, in the same
 * operation order (a side with count 0 is skipped, not multiplied through), so
 * results are bit-identical from run to run.  The m2s are clamped at 0, cxy is
 * not.  An unmasked NaN or +-inf on either side of a counted pair gives a NaN
 * cxy (and a NaN m2 on that side). */
typedef struct { int64_t count; double mean_x, mean_y, m2_x, m2_y, cxy; } pyas_comoments;

/* pyas_moments_axes over two variables: chunk c of y pairs with chunk c of x.
 * x and y must agree in ndim, chunk_shape and n_chunks (PYAS_EINVAL) and in
 * dtype (PYAS_ENOTSUP).  sel and index_pool are read from x only: y's are
 * ignored, the selection of both sides is x's.  data, offsets, shuffle,
 * byteswap and the mask are per side; a pair counts when neither mask_x masks
 * its x nor mask_y its y, and the mask tables of each side are indexed by the
 * same selection position.  Outputs, out_offsets and the other errors as
 * pyas_moments_axes; PYAS_EINVAL when a batch is NULL.  With every dim in
 * axes_mask a selection that is one contiguous run streams both buffers with
 * 16-byte loads when both chunk bases are misaligned alike (base & 15), and is
 * walked per element otherwise. */
int pyas_comoments_axes(pyas_ctx *ctx, const pyas_batch *x, const pyas_mask *mask_x,
                        const pyas_batch *y, const pyas_mask *mask_y, uint32_t axes_mask,
                        const int64_t *out_offsets, pyas_comoments *out, void *stream);
/* pyas_moments_combine_segments / pyas_moments_combine_grid for comoments
 * records (same orders, same errors). */
int pyas_comoments_combine_segments(pyas_ctx *ctx, const pyas_comoments *in, const int64_t *index,
                                    const int64_t *seg_offsets, int64_t n_segments,
                                    pyas_comoments *out, void *stream);
int pyas_comoments_combine_grid(pyas_ctx *ctx, const pyas_comoments *in, const pyas_grid *grid,
                                pyas_comoments *out, void *stream);

/* ---- least-squares trend against a coordinate (Active.trend) ----------------
 * The pyas_comoments record with x a coordinate instead of a second stored
 * variable: for an element of chunk c at index i inside the chunk along chunk
 * dim `dim`, x = pool[origin[c] + i] and y is the data value (converted to f64
 * as astype(float64) does); the pair counts when y is unmasked.  Slices,
 * strides and index lists look up the same way (by the element's index inside
 * the chunk).  Every coordinate of a chunk must be readable:
 * pool[origin[c] .. + chunk_shape[dim]).  This is the single-dim form of
 * pyas_weights.  Lanes accumulate and records merge exactly as for
 * pyas_comoments_axes, so slope = cxy / m2_x, intercept = mean_y - slope mean_x,
 * and pyas_comoments_combine_segments / _grid combine the records. */
typedef struct {
    const double *pool;      /* device: the coordinate vector, zero-padded to whole chunks */
    const int32_t *origin;   /* device [n_chunks]: index in pool of chunk c's local index 0 along dim */
    int32_t dim;             /* the chunk dim the coordinate runs along; must be in the reduced dims */
} pyas_coord;

/* pyas_comoments_axes against a coordinate: outputs, out_offsets and errors as
 * there (out_offsets may be NULL only with every dim in axes_mask); PYAS_EINVAL
 * when coord or one of its pointers is NULL or coord->dim is not a reduced dim.
 * A per-element walk for any selection and mask: it has no speed target. */
int pyas_trend_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_coord *coord, uint32_t axes_mask, const int64_t *out_offsets,
                    pyas_comoments *out, void *stream);
/* The dense path of a box query: pyas_trend_axes + pyas_comoments_combine_grid
 * in ONE launch that writes one finished record per final output (out, device,
 * C order over grid->out_extent) and no per-chunk records.  The caller promises
 * a unit-step box: every dim's selection is one unit-step range of the
 * variable (batch->sel NULL: whole chunks), the chunks are laid out in the
 * grid's C order (chunk n = grid position n, prod n_coords chunks) and chunks
 * that share a dim's chunk coordinate share that dim's selection.  Only
 * grid->ndim, axes_mask, n_coords and out_extent are read.  The reduced dims
 * must be a leading prefix 0 .. P-1 of the dims with at least one kept dim
 * behind them, and the mask must have no vector tables: otherwise
 * PYAS_ENOTSUP, nothing is launched and the caller takes pyas_trend_axes.
 * A lane owns 4 consecutive outputs along the innermost dim and walks them
 * through every row of every chunk layer in increasing index order, so a
 * record is the lane's own sums (nothing is merged).  Records differ from the
 * two-step path's in the last bits (another summation order); both are
 * bit-identical from run to run. */
int pyas_trend_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_coord *coord, const pyas_grid *grid, pyas_comoments *out,
                    void *stream);
/* value[i] = cxy / m2_x (PYAS_TREND_SLOPE) or mean_y - slope mean_x
 * (PYAS_TREND_INTERCEPT, one fma) of record i, masked[i] = (count == 0), all
 * device: 9 bytes per output cross PCIe instead of 48.  A masked value is 0;
 * m2_x == 0 gives NaN (0 / 0), unmasked. */
enum { PYAS_TREND_SLOPE = 0, PYAS_TREND_INTERCEPT = 1 };
int pyas_trend_finalize(pyas_ctx *ctx, const pyas_comoments *in, int64_t n, int32_t what,
                        double *value, uint8_t *masked, void *stream);

/* ---- spells past a threshold (Active.spell) -----------------------------------
 * Partial record of the runs of true elements in a sequence of selected
 * positions along one dim (40 bytes, ten int32).  A position is true when its
 * element is unmasked and float64(x) op threshold holds (values convert as
 * astype(float64) does; a NaN compares false but counts as unmasked); a masked
 * element is false.  A run is a maximal sequence of consecutive true positions.
 *   n, n_true   unmasked / true positions
 *   len         positions covered
 *   head, tail  length of the leading / trailing run (both == len when every
 *               position is true)
 *   best        longest run anywhere
 *   days, events  total length / number of the interior runs of length >=
 *               min_length (an interior run touches neither end of the sequence)
 *   min_length  the query's L (0 in the zero record)
 * The all-zero record is neutral.  Unlike the other records this one merges in
 * sequence order only: merged(a, b) with a's positions before b's,
 *   L = max(a.min_length, b.min_length); a_all = a.head == a.len; b_all likewise
 *   n, n_true, len add
 *   head = a_all ? a.len + b.head : a.head;  tail = b_all ? b.len + a.tail : b.tail
 *   j = a.tail + b.head;  best = max(a.best, b.best, j)
 *   days, events add; and when !a_all && !b_all && j >= L: days += j, events += 1
 * is associative but not commutative.  Every combine of the library folds its
 * records sequentially in a fixed order (a segment in index order, chunk layers
 * in C order over the reduced dim's chunk coordinates), so the caller hands
 * the records over in sequence order and nothing else is needed.  Finalize:
 *   longest = best
 *   events += (head >= L && head > 0) + (head != len && tail >= L && tail > 0)
 *   days   += (head >= L ? head : 0) + (head != len && tail >= L ? tail : 0)
 * All counts are int32: a sequence holds fewer than 2^31 positions. */
typedef struct {
    int32_t n, n_true, len, head, tail, best, days, events, min_length, reserved;
} pyas_spell;

enum { PYAS_SPELL_GT = 0, PYAS_SPELL_GE = 1, PYAS_SPELL_LT = 2, PYAS_SPELL_LE = 3 };
enum { PYAS_SPELL_LONGEST = 0, PYAS_SPELL_DAYS = 1, PYAS_SPELL_EVENTS = 2 };
typedef struct {
    int32_t dim;             /* the chunk dim the runs follow: the one reduced dim */
    int32_t op;              /* PYAS_SPELL_GT / GE / LT / LE */
    int32_t min_length;      /* L >= 1 */
    double threshold;        /* finite */
} pyas_spell_rule;

/* pyas_moments_axes for spell records: out[out_offsets[c] + o] receives the
 * record of output o (C order over the kept selected dims) of chunk c, over the
 * chunk's selected positions along rule->dim in selection order (a slice by
 * its step, an index list in list order: the host passes increasing lists).
 * axes_mask must be 1u << rule->dim; op must be one of the four and
 * min_length >= 1 (PYAS_EINVAL otherwise, and when rule is NULL).  out_offsets
 * may be NULL only for a 1-D variable (chunk c's record at out[c]).  When
 * rule->dim is the innermost dim a wave owns an output and takes 64
 * consecutive positions per step (two ballots and bit operations give the
 * word's record, merged into the wave's in word order); otherwise a lane walks
 * its output's positions in order.  A per-element walk for any selection and
 * mask: it has no speed target.  Other errors as pyas_moments_axes. */
int pyas_spell_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_spell_rule *rule, uint32_t axes_mask, const int64_t *out_offsets,
                    pyas_spell *out, void *stream);
/* The dense path of a box query: pyas_spell_axes + pyas_spell_combine_grid in
 * ONE launch that writes one finished record per final output (out, device, C
 * order over grid->out_extent) and no per-chunk records.  The caller's promises
 * and the grid fields read are those of pyas_trend_cols.  rule->dim must be 0,
 * the single reduced dim (grid->axes_mask == 1), with at least one kept dim
 * behind it, and the mask must have no vector tables: otherwise PYAS_ENOTSUP,
 * nothing is launched and the caller takes pyas_spell_axes.  A lane owns 4
 * consecutive outputs along the innermost dim and walks them through every row
 * of every chunk layer in increasing index order, keeping the current run, the
 * head and the counts in integer registers, so a record is the lane's own
 * (nothing is merged) and equals the two-step path's exactly. */
int pyas_spell_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_spell_rule *rule, const pyas_grid *grid, pyas_spell *out,
                    void *stream);
/* pyas_moments_combine_segments / pyas_moments_combine_grid for spell records
 * (same orders, same errors).  The records of a segment must be listed, and
 * the chunk layers must lie, in sequence order. */
int pyas_spell_combine_segments(pyas_ctx *ctx, const pyas_spell *in, const int64_t *index,
                                const int64_t *seg_offsets, int64_t n_segments,
                                pyas_spell *out, void *stream);
int pyas_spell_combine_grid(pyas_ctx *ctx, const pyas_spell *in, const pyas_grid *grid,
                            pyas_spell *out, void *stream);
/* value[i] = the finalized longest / days / events (stat: PYAS_SPELL_*) of
 * record i as int32, masked[i] = (n == 0), all device: 5 bytes per output cross
 * PCIe instead of 40.  A masked value is 0. */
int pyas_spell_finalize(pyas_ctx *ctx, const pyas_spell *in, int64_t n, int32_t stat,
                        int32_t *value, uint8_t *masked, void *stream);

/* ---- where the extreme lies (Active.argmax / Active.argmin) -------------------
 * Partial record of the arg-extreme of a set of selected positions along one
 * dim (16 bytes): the winning unmasked element.
 *   value   the winner itself in the data's class, as in pyas_partial (f for
 *           floats, carried exactly as f64; i for signed, u for unsigned
 *           integers), the stored element untouched: the sign of a zero and a
 *           NaN are the element's own
 *   index   its global index along the dim (origin[c] + the index in chunk c)
 *   n       unmasked positions
 * Element b beats element a when b is a NaN and a is not, or when neither is a
 * NaN and b > a (PYAS_ARGEXT_MAX) / b < a (PYAS_ARGEXT_MIN) compared in the
 * data's class (8-byte integers exactly; -0.0 == +0.0); among equals, and
 * between two NaNs, the smaller index wins (and at one index, which is one
 * element, the smaller bit pattern: the order is total).  Masked elements take
 * no part.
 * The all-zero record is neutral, and so is every record with n == 0 (its
 * other fields are written as 0).  merged(a, b): the winner of the two by the
 * rule above, n adds.  The rule is a total order on (value, index), so the
 * merge is associative and commutative: the combines may take the records in
 * any order and give the same record.  index and n are int32: the dim holds
 * fewer than 2^31 indices. */
typedef struct {
    pyas_scalar value;
    int32_t index;
    int32_t n;
} pyas_argext;

enum { PYAS_ARGEXT_MAX = 0, PYAS_ARGEXT_MIN = 1 };
typedef struct {
    int32_t dim;             /* the chunk dim the index runs along: the one reduced dim */
    int32_t which;           /* PYAS_ARGEXT_MAX / PYAS_ARGEXT_MIN */
    const int32_t *origin;   /* device [n_chunks]: global index along dim of chunk c's local index 0
                              * (the chunk coordinate times the chunk extent, as pyas_coord.origin) */
} pyas_argext_rule;

/* pyas_spell_axes for argext records: out[out_offsets[c] + o] receives the
 * record of output o (C order over the kept selected dims) of chunk c, over the
 * chunk's selected positions along rule->dim.  axes_mask must be
 * 1u << rule->dim; which must be one of the two and origin non-NULL
 * (PYAS_EINVAL otherwise, and when rule is NULL).  out_offsets may be NULL only
 * for a 1-D variable (chunk c's record at out[c]).  When rule->dim is the
 * innermost dim a wave owns an output: lane k takes positions k, k + 64, ...
 * and the lanes' records are merged with shuffles (the merge is commutative);
 * otherwise a lane walks its output's positions.  A per-element walk for any
 * selection and mask: it has no speed target.  Other errors as
 * pyas_moments_axes. */
int pyas_argext_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                     const pyas_argext_rule *rule, uint32_t axes_mask, const int64_t *out_offsets,
                     pyas_argext *out, void *stream);
/* The dense path of a box query: pyas_argext_axes + pyas_argext_combine_grid in
 * ONE launch that writes one finished record per final output (out, device, C
 * order over grid->out_extent) and no per-chunk records.  The caller's promises
 * and the grid fields read are those of pyas_trend_cols.  rule->dim must be 0,
 * the single reduced dim (grid->axes_mask == 1), with at least one kept dim
 * behind it, and the mask must have no vector tables: otherwise PYAS_ENOTSUP,
 * nothing is launched and the caller takes pyas_argext_axes.  A lane owns 4
 * consecutive outputs along the innermost dim and walks them through every row
 * of every chunk layer in increasing index order, keeping the best value, its
 * row and the count in registers (updated by selects; a strict "beats" keeps
 * the first occurrence), so a record is the lane's own (nothing is merged) and
 * equals the two-step path's exactly. */
int pyas_argext_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                     const pyas_argext_rule *rule, const pyas_grid *grid, pyas_argext *out,
                     void *stream);
/* pyas_moments_combine_segments / pyas_moments_combine_grid for argext records
 * (same orders, same errors).  The merge compares values in the data's class,
 * so both take the data's dtype (pyas_dtype; PYAS_ENOTSUP when it is none of
 * the ten) and which (PYAS_EINVAL when it is neither of the two). */
int pyas_argext_combine_segments(pyas_ctx *ctx, int32_t dtype, int32_t which, const pyas_argext *in,
                                 const int64_t *index, const int64_t *seg_offsets, int64_t n_segments,
                                 pyas_argext *out, void *stream);
int pyas_argext_combine_grid(pyas_ctx *ctx, int32_t dtype, int32_t which, const pyas_argext *in,
                             const pyas_grid *grid, pyas_argext *out, void *stream);
/* index[i] = the index of record i as int32, masked[i] = (n == 0), all device:
 * 5 bytes per output cross PCIe instead of 16.  A masked index is 0. */
int pyas_argext_finalize(pyas_ctx *ctx, const pyas_argext *in, int64_t n, int32_t *index,
                         uint8_t *masked, void *stream);

/* ---- conditional reductions past a threshold (Active.exceed) ------------------
 * Partial record of the selected positions of an output (32 bytes).  A position
 * is true when its element is unmasked and float64(x) op t holds, t the
 * output's threshold (values convert as astype(float64) does; a NaN element
 * compares false but counts as unmasked; a masked element is false; a NaN
 * threshold, which is how the host hands over a masked field entry, makes
 * nothing true).
 *   n        unmasked positions
 *   n_true   true positions
 *   sum      sum of float64(x) over the true positions, in f64 from the first
 *            addition
 *   excess   sum over the true positions of one f64 subtraction each: x - t for
 *            GT / GE, t - x for LT / LE (never derived from sum - t n_true)
 * The all-zero record is neutral; merged(a, b) adds field by field.  The
 * integer fields are exact on every path; sum and excess depend on the order of
 * the additions in the last bits, and every kernel and combine of the library
 * adds in a fixed order, so a result is bit-identical from run to run. */
typedef struct {
    int64_t n;
    int64_t n_true;
    double sum;
    double excess;
} pyas_exceed;

/* A threshold per output: the field as the caller gave it, in C order over its
 * own shape (the variable's extent on every kept dim, 1 on every reduced dim).
 * The threshold of an output of chunk c whose kept dims' indices inside the
 * chunk are local[d] is values[origin[c] + sum_d local[d] * stride[d]]. */
typedef struct {
    const double *values;    /* device: the field; NaN where an entry is masked */
    const int64_t *origin;   /* device [n_chunks]: the field offset of chunk c's local index 0 */
    int64_t stride[PYAS_MAX_DIMS];   /* field element stride per dim; 0 on reduced dims */
} pyas_exceed_field;

enum { PYAS_EXCEED_COUNT = 0, PYAS_EXCEED_FRACTION = 1, PYAS_EXCEED_SUM = 2, PYAS_EXCEED_MEAN = 3,
       PYAS_EXCEED_EXCESS = 4 };
typedef struct {
    int32_t op;              /* PYAS_SPELL_GT / GE / LT / LE */
    int32_t reserved;
    double threshold;        /* finite; read when field is NULL */
    const pyas_exceed_field *field;   /* NULL: one threshold for every output */
} pyas_exceed_rule;

/* pyas_moments_axes for exceed records: out[out_offsets[c] + o] receives the
 * record of output o (C order over the kept selected dims) of chunk c over the
 * chunk's selected positions along the dims of axes_mask, any subset of the
 * dims.  op must be one of the four; a scalar threshold must be finite; a field
 * needs both tables and is refused when every dim is reduced (a field of one
 * entry is a scalar): PYAS_EINVAL otherwise, and when rule is NULL.  With every
 * dim reduced a workgroup takes a tile of a chunk (a contiguous selection
 * streams 16-B loads) and the tiles are merged in tile order; out_offsets may
 * then be NULL (chunk c's record at out[c]).  Otherwise a lane owns an output
 * when the innermost dim is kept and a wave owns it when that dim is reduced
 * (lanes merged with shuffles in a fixed order); the output's threshold is
 * loaded once per output.  Other errors as pyas_moments_axes. */
int pyas_exceed_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                     const pyas_exceed_rule *rule, uint32_t axes_mask, const int64_t *out_offsets,
                     pyas_exceed *out, void *stream);
/* The dense path of a box query: pyas_exceed_axes + pyas_exceed_combine_grid in
 * ONE launch that writes one finished record per final output (out, device, C
 * order over grid->out_extent) and no per-chunk records.  The caller's promises,
 * the grid fields read and the geometries served are those of pyas_trend_cols:
 * the reduced dims are a leading prefix 0 .. P-1 of the dims with at least one
 * kept dim behind them, the mask has no vector tables, and an output covers
 * fewer than 2^32 chunk positions: otherwise PYAS_ENOTSUP, nothing is launched
 * and the caller takes pyas_exceed_axes.  A lane owns 4 consecutive outputs
 * along the innermost dim, loads their 4 thresholds once (from the field by
 * the formula above) and walks them through every row of every chunk layer in
 * increasing index order, so a record is the lane's own (nothing is merged).
 * n and n_true equal the two-step path's; sum and excess may differ from it in
 * the last bits (another summation order). */
int pyas_exceed_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                     const pyas_exceed_rule *rule, const pyas_grid *grid, pyas_exceed *out,
                     void *stream);
/* pyas_moments_combine_segments / pyas_moments_combine_grid for exceed records
 * (same orders, same errors). */
int pyas_exceed_combine_segments(pyas_ctx *ctx, const pyas_exceed *in, const int64_t *index,
                                 const int64_t *seg_offsets, int64_t n_segments,
                                 pyas_exceed *out, void *stream);
int pyas_exceed_combine_grid(pyas_ctx *ctx, const pyas_exceed *in, const pyas_grid *grid,
                             pyas_exceed *out, void *stream);
/* One statistic (stat: PYAS_EXCEED_*) of n records, all device: 8 bytes at
 * value + 8 i (an int64 for COUNT, a double for the rest) and the byte
 * masked[i], so 9 bytes per output cross PCIe instead of 32.
 *   COUNT n_true, FRACTION n_true / n, SUM sum, EXCESS excess: masked when n == 0
 *   MEAN sum / n_true: masked when n_true == 0
 * and masked as well where thr_masked[i] != 0 (device, one byte per output:
 * the output's threshold is masked; NULL: none is).  A masked value is 0. */
int pyas_exceed_finalize(pyas_ctx *ctx, const pyas_exceed *in, int64_t n, int32_t stat,
                         const uint8_t *thr_masked, void *value, uint8_t *masked, void *stream);

/* ---- running-window extremes (Active.rolling) ---------------------------------
 * Partial record of the extreme window sum of a sequence of selected positions
 * along one dim (144 bytes).  A window is w positions consecutive in the
 * selection; it is valid when all w elements are unmasked (a NaN is data, not
 * a masked element).  A valid window's sum is
 *   s = f64(x[p]); s += f64(x[p+1]); ...; s += f64(x[p+w-1])
 * (each element converts as astype(float64) does; w - 1 float64 additions,
 * oldest element first: this order is the definition, nothing is added and
 * subtracted along the way).  The extreme keeps the first among equal sums
 * (-0.0 == +0.0) and the first NaN sum wins, as in np.max / np.min.
 *   best         the extreme valid-window sum (0 when n_windows == 0)
 *   position     of that window's first element within the piece (0 when none)
 *   n_windows    valid windows
 *   n, len       unmasked positions / positions
 *   window       w (1 .. PYAS_ROLL_MAX_WINDOW), which: PYAS_ROLL_MAX / MIN; both
 *                travel in the record so that a merge needs no argument
 *   head[j]      the piece's element j, j < min(len, w - 1)
 *   tail[k]      the piece's element len - 1 - k, k < min(len, w - 1): the LAST
 *                element is tail[0]
 *   head_ok, tail_ok   bit j: head[j] / tail[j] exists and is unmasked
 * Slots that do not exist or are masked hold 0 and a clear bit, so equal
 * pieces give equal bytes.  The all-zero record is neutral on either side.
 * Merge (a before b, NOT commutative, associative), w = max of the windows:
 *   every window of m = w-1 .. 1 elements of a's end and w - m of b's start
 *   (valid when tail_ok bits 0 .. m-1 and head_ok bits 0 .. w-m-1 are set) is
 *   summed by the rule above, at position a.len - m; the candidates a.best,
 *   those windows by decreasing m, b.best (position + a.len) are taken in
 *   this order, a later one winning only when it strictly beats a non-NaN
 *   holder or is the first NaN; the counts add; head = the first
 *   min(len, w-1) of a.head ++ b.head, tail likewise from the end.
 * All counts are int32: a sequence holds fewer than 2^31 positions. */
#define PYAS_ROLL_MAX_WINDOW 8
typedef struct {
    double best;
    int32_t position, n_windows, n, len;
    uint8_t window, which, head_ok, tail_ok;
    int32_t reserved;
    double head[PYAS_ROLL_MAX_WINDOW - 1], tail[PYAS_ROLL_MAX_WINDOW - 1];
} pyas_roll;

enum { PYAS_ROLL_MAX = 0, PYAS_ROLL_MIN = 1 };
enum { PYAS_ROLL_SUM = 0, PYAS_ROLL_MEAN = 1 };
typedef struct {
    int32_t dim;             /* the chunk dim the windows follow: the one reduced dim */
    int32_t window;          /* 1 .. PYAS_ROLL_MAX_WINDOW */
    int32_t which;           /* PYAS_ROLL_MAX / PYAS_ROLL_MIN */
} pyas_roll_rule;

/* pyas_spell_axes for roll records: out[out_offsets[c] + o] receives the record
 * of output o (C order over the kept selected dims) of chunk c, over the
 * chunk's selected positions along rule->dim in selection order.  axes_mask
 * must be 1u << rule->dim, window in 1 .. PYAS_ROLL_MAX_WINDOW and which one of
 * the two (PYAS_EINVAL otherwise, and when rule is NULL).  out_offsets may be
 * NULL only for a 1-D variable (chunk c's record at out[c]).  A lane walks its
 * output's positions in order, whichever dim the windows follow: a
 * per-element walk for any selection and mask, with no speed target.  Other
 * errors as pyas_moments_axes. */
int pyas_roll_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                   const pyas_roll_rule *rule, uint32_t axes_mask, const int64_t *out_offsets,
                   pyas_roll *out, void *stream);
/* The dense path of a box query, as pyas_spell_cols (same promises, same grid
 * fields, same PYAS_ENOTSUP cases with nothing launched): one launch writes
 * one finished record per final output.  A lane owns 4 consecutive outputs
 * along the innermost dim and walks them through every row of every chunk
 * layer in increasing index order with the previous w - 1 elements of each in
 * registers, so every window sum is formed by the same additions as
 * pyas_roll_axes followed by the combines form it: the records are equal byte
 * for byte. */
int pyas_roll_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                   const pyas_roll_rule *rule, const pyas_grid *grid, pyas_roll *out,
                   void *stream);
/* pyas_spell_combine_segments / pyas_spell_combine_grid for roll records (same
 * orders, same errors): the records of a segment must be listed, and the chunk
 * layers must lie, in sequence order. */
int pyas_roll_combine_segments(pyas_ctx *ctx, const pyas_roll *in, const int64_t *index,
                               const int64_t *seg_offsets, int64_t n_segments,
                               pyas_roll *out, void *stream);
int pyas_roll_combine_grid(pyas_ctx *ctx, const pyas_roll *in, const pyas_grid *grid,
                           pyas_roll *out, void *stream);
/* value[i] = best (stat PYAS_ROLL_SUM) or best / float64(window)
 * (PYAS_ROLL_MEAN) of record i, masked[i] = (n_windows == 0), all device: 9
 * bytes per output cross PCIe instead of 144.  A masked value is 0. */
int pyas_roll_finalize(pyas_ctx *ctx, const pyas_roll *in, int64_t n, int32_t stat,
                       double *value, uint8_t *masked, void *stream);

/* ---- per-label second moments (Active.grouped) -------------------------------
 * The pyas_moments record, one per (output, group): an element whose global
 * index along one reduced dim is i belongs to group labels[i] >= 0, or to no
 * group (labels[i] < 0).  The host turns the labels into the tables below;
 * like the selection table they are trusted (the host builds and checks
 * them).  Lanes accumulate exactly as for pyas_moments_axes. */

/* The reduced rows of a unit-step box query, for pyas_group_cols.  A row is
 * one position of the reduced (leading) dims' selection: its chunk layer (the
 * C-order position of its chunk over the reduced dims' chunk coordinates), its
 * element offset inside the chunk (sum over the reduced dims of the index
 * inside the chunk times the chunk's element stride) and its label.  Only
 * rows with a label >= 0 are listed, sorted by label (stably: in increasing
 * global order inside a label), so every group is one run.  Every column of
 * chunks walks the same list. */
typedef struct {
    const int32_t *layer;    /* device [n_rows] */
    const int32_t *offset;   /* device [n_rows] */
    const int32_t *label;    /* device [n_rows]: non-decreasing, in [0, n_groups) */
    int64_t n_rows;          /* 0: every record is the zero record (the pointers may be NULL) */
    int32_t n_groups;
} pyas_group_rows;
#define PYAS_GROUP_ROWS 1024 /* rows of the list a workgroup of pyas_group_cols stages per pass */

/* The dense path of a box query, in ONE launch: out[g * n_out + o] (device;
 * o in C order over grid->out_extent, n_out = their product) receives the
 * finished record of final output o over the rows of group g, for every g in
 * [0, n_groups): the zero record where the group has no row.  The kernel
 * writes every one of these records, so `out` needs no initialisation.  The
 * caller's promises, the geometries taken and PYAS_ENOTSUP (nothing launched;
 * the caller takes pyas_group_axes) are those of pyas_trend_cols; rows->n_rows
 * < 0 or n_groups < 0 is PYAS_EINVAL, n_groups == 0 launches nothing.  A lane
 * owns 4 consecutive outputs along the innermost dim and walks the list in
 * order; at a change of label it stores its 4 records and starts again, so a
 * record is the lane's own sums over all chunk layers (nothing is merged) and
 * results are bit-identical from run to run.  Rows that are not listed are
 * never read. */
int pyas_group_cols(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_group_rows *rows, const pyas_grid *grid, pyas_moments *out,
                    void *stream);

/* The groups of each chunk, for pyas_group_axes (CSR): chunk c has the local
 * groups chunk_start[c] .. chunk_start[c+1]; local group j holds the positions
 * pos[ptr[j] .. ptr[j+1]) among the chunk's SELECTED indices along chunk dim
 * `dim` (position k is the k-th entry of the dim's selection in the chunk, the
 * index the selection table and the mask tables' strides see), increasing. */
typedef struct {
    const int32_t *chunk_start;   /* device [n_chunks + 1] */
    const int32_t *ptr;           /* device [n_local_groups + 1] */
    const int32_t *pos;           /* device */
    int32_t dim;                  /* must be in the reduced dims */
} pyas_group_lists;

/* pyas_moments_axes with one record per (chunk output, chunk-local group):
 * out[out_offsets[c] + j * n_keep + o] receives the record of output o (C
 * order over the n_keep kept selected positions of chunk c) over local group
 * j of chunk c (j from 0).  Errors as pyas_trend_axes (lists for coord; out_offsets
 * is always needed).  pyas_moments_combine_segments merges the records.  A
 * per-element walk for any selection and mask: it has no speed target. */
int pyas_group_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                    const pyas_group_lists *lists, uint32_t axes_mask, const int64_t *out_offsets,
                    pyas_moments *out, void *stream);

/* ---- per-label sums and extremes (Active.grouped "min" / "max" / "sum") -------
 * pyas_group_cols and pyas_group_axes over pyas_partial records: per (output,
 * group) the sum (f64 from the first addition for floats, int64 / uint64
 * wrapping modulo 2^64 for ints), the count, and the NaN-propagating min and
 * max compared in the variable's type.  The same tables, promises and error
 * codes; no atomics, every record written once by its owner. */

/* pyas_group_cols for partial records: out[g * n_out + o] is the finished
 * record of every (group, output); the ALL-ZERO record where group g has no
 * row (count == 0: min and max are meaningless), so `out` needs no zeroing.
 * PYAS_ENOTSUP for exactly the geometries pyas_group_cols refuses. */
int pyas_group_cols_partial(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                            const pyas_group_rows *rows, const pyas_grid *grid, pyas_partial *out,
                            void *stream);

/* pyas_group_axes for partial records: one record per (chunk output,
 * chunk-local group) at out[out_offsets[c] + j * n_keep + o].
 * pyas_combine_segments with combine_flags = 0 merges them. */
int pyas_group_axes_partial(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                            const pyas_group_lists *lists, uint32_t axes_mask,
                            const int64_t *out_offsets, pyas_partial *out, void *stream);

/* ---- weighted sums (Active.mean / Active.sum with weights=) -----------------
 * Partial record of a weighted mean over a set of elements (32 bytes):
 * count unmasked elements; sw = sum w; swx = sum w x  (f64).  The all-zero
 * record is neutral and records merge by plain f64 addition of each field, in
 * the fixed order of the moments records (lanes pairwise at distance 1, 2,
 * 4..., waves in wave order, tiles in tile order, chunks in the order of the
 * combines), so results are bit-identical from run to run.
 * The weight of an element is the product of one factor per chunk dim,
 *   w = ((1 * f_0) * f_1) * ... * f_{ndim-1},   f_d = pool[origin[c][d] + i_d],
 * multiplied in ascending dim order (the leading 1 is exact), where i_d is the
 * element's index inside chunk c along dim d: slices, strides and index lists
 * look up the same way.  A dim without weights points at a run of 1.0.  Every
 * factor of a chunk must be readable: pool[origin[c][d] .. + chunk_shape[d]).
 * x converts to f64 as astype(float64) does; a lane adds w to sw and
 * fma(w, x, swx) to swx.  Masked elements are excluded by select, never
 * multiplied by 0; an unmasked NaN gives a NaN swx. */
typedef struct { int64_t count; double sw; double swx; uint64_t reserved; } pyas_wsum;

typedef struct {
    const double *pool;      /* device: the per-dim factor vectors, concatenated */
    const int32_t *origin;   /* device [n_chunks * PYAS_MAX_DIMS]: index in pool of the factor
                                of chunk c's local index 0 along dim d */
} pyas_weights;

/* pyas_moments_axes for weighted sums: same outputs, out_offsets and errors;
 * PYAS_EINVAL when weights or one of its pointers is NULL. */
int pyas_wsum_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                   const pyas_weights *weights, uint32_t axes_mask, const int64_t *out_offsets,
                   pyas_wsum *out, void *stream);
/* pyas_combine_segments / pyas_combine_grid for weighted-sum records (same orders). */
int pyas_wsum_combine_segments(pyas_ctx *ctx, const pyas_wsum *in, const int64_t *index,
                               const int64_t *seg_offsets, int64_t n_segments, pyas_wsum *out,
                               void *stream);
int pyas_wsum_combine_grid(pyas_ctx *ctx, const pyas_wsum *in, const pyas_grid *grid,
                           pyas_wsum *out, void *stream);

/* ---- weighted second moments (Active.var / std / cov / corr with weights=) ----
 * Partial record of a weighted covariance over a set of pairs (64 bytes):
 * count pairs unmasked on both sides; sw = sum w and sw2 = sum w^2 over them;
 * mean_x = sum w x / sw and mean_y; m2_x = sum w (x - mean_x)^2, m2_y likewise
 * and cxy = sum w (x - mean_x)(y - mean_y)  (all in f64; the weights as for
 * pyas_wsum, values converted as astype(float64) does).  The all-zero record is
 * neutral.  One pass: each lane keeps shifts Kx, Ky (its first counted pair of
 * weight > 0; 0 before it, where every term has weight exactly 0) with
 * sum w (x-Kx), sum w (x-Kx)^2, sum w (y-Ky), sum w (y-Ky)^2 and
 * sum w (x-Kx)(y-Ky) in f64 (FMA), and finishes to mean = K + s1/sw,
 * m2 = s2 - s1^2/sw (sw == 0: mean 0, m2 = s2).  Lanes, waves, tiles and chunks
 * merge a then b in the fixed order of the moments records: count, sw and sw2
 * add; when both sw > 0,
 *   d_x = mean_x_b - mean_x_a;  f = sw_b / (sw_a + sw_b);
 *   mean_x = mean_x_a + d_x f;  m2_x = m2_x_a + m2_x_b + d_x d_x sw_a f;
 *   cxy = cxy_a + cxy_b + d_x d_y sw_a f
 * (y likewise); a side with sw == 0 gives no mean, but its m2_x, m2_y and cxy
 * (each exactly 0, or NaN) are still added, so results are bit-identical from
 * run to run.  The m2s are clamped at 0, cxy is not.  A counted NaN or +-inf on
 * either side gives a NaN cxy (and a NaN m2 on that side) at any weight,
 * exactly 0 included; masked elements are excluded by select and never reach a
 * product. */
typedef struct {
    int64_t count;
    double sw, sw2, mean_x, mean_y, m2_x, m2_y, cxy;
} pyas_wcomoments;

/* pyas_comoments_axes with weights.  y == NULL (mask_y ignored): one variable;
 * mean_y, m2_y and cxy are written 0 and no second buffer is read.  Otherwise x
 * and y must agree as for pyas_comoments_axes (PYAS_EINVAL; dtypes
 * PYAS_ENOTSUP) and the selection of both sides is x's.  PYAS_EINVAL when
 * weights or one of its pointers is NULL.  Outputs, out_offsets and the other
 * errors as pyas_moments_axes.  With every dim in axes_mask a selection that is
 * one contiguous run streams 16-byte loads when the two sides agree in shuffle
 * and their chunk bases are misaligned alike (base & 15), and is walked per
 * element otherwise. */
int pyas_wcomoments_axes(pyas_ctx *ctx, const pyas_batch *x, const pyas_mask *mask_x,
                         const pyas_batch *y, const pyas_mask *mask_y, const pyas_weights *weights,
                         uint32_t axes_mask, const int64_t *out_offsets, pyas_wcomoments *out,
                         void *stream);
/* pyas_moments_combine_segments / pyas_moments_combine_grid for wcomoments
 * records (same orders, same errors). */
int pyas_wcomoments_combine_segments(pyas_ctx *ctx, const pyas_wcomoments *in, const int64_t *index,
                                     const int64_t *seg_offsets, int64_t n_segments,
                                     pyas_wcomoments *out, void *stream);
int pyas_wcomoments_combine_grid(pyas_ctx *ctx, const pyas_wcomoments *in, const pyas_grid *grid,
                                 pyas_wcomoments *out, void *stream);

/* ---- binned counts (Active.histogram) -----------------------------------------
 * Bin rule, over n_bins + 1 strictly increasing finite f64 edges e: an
 * unmasked selected element x (converted to f64 as astype(float64) does)
 * counts in bin i when e[i] <= x < e[i+1]; the last bin also holds
 * x == e[n_bins]; x < e[0] and -inf count as `below`, x > e[n_bins] and +inf
 * as `above`, NaN as `nan`.  Masked elements count nowhere.
 * Table row of one output: n_bins counts, then below, above, nan: n_bins + 3
 * int64.  Counts are added to the table, which the caller zeroes
 * (pyas_hist_reset); integer adds commute, so results are exact and
 * bit-identical from run to run.
 * For uniform edges (PYAS_HIST_UNIFORM) the kernels guess the bin as
 * (x - lo) * scale, lo = e[0], scale = n_bins / (e[n_bins] - e[0]); the guess is
 * only a starting point, the edge table decides. */
#define PYAS_HIST_UNIFORM 1u
#define PYAS_HIST_MAX_BINS (1 << 20)
typedef struct {
    const double *edges;     /* device: n_bins + 1 edges */
    int32_t n_bins;
    uint32_t flags;          /* PYAS_HIST_* */
    double lo;               /* PYAS_HIST_UNIFORM: e[0] */
    double scale;            /* PYAS_HIST_UNIFORM: n_bins / (e[n_bins] - e[0]) */
} pyas_hist;

/* pyas_moments_axes for binned counts (same argument checks and errors):
 * output o (C order over the kept selected dims) of chunk c adds into table
 * row out_index[out_offsets[c] + o], or row out_offsets[c] + o when out_index
 * is NULL (both device).  With every dim in axes_mask a chunk has one output
 * and out_offsets may be NULL: every chunk adds into row 0; up to 2,048 bins
 * count in LDS and each workgroup adds its table once.  PYAS_EINVAL when hist,
 * its edges or table is NULL, n_bins < 1 or n_bins > PYAS_HIST_MAX_BINS. */
int pyas_hist_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                   const pyas_hist *hist, uint32_t axes_mask, const int64_t *out_offsets,
                   const int64_t *out_index, int64_t *table, void *stream);
/* Zero n_rows table rows of n_bins + 3 int64 on the stream. */
int pyas_hist_reset(pyas_ctx *ctx, int64_t *table, int64_t n_rows, int32_t n_bins, void *stream);

/* ---- exact order statistics (Active.quantile) --------------------------------
 * The k-th smallest unmasked selected element of every output, by a radix
 * select over keys, most significant digit first.
 * Key rule: every element maps to an unsigned key in the order of the values;
 * a caller inverts it to read the element back.
 *   u8, u16, u32   32-bit key: the value, zero-extended.
 *   i8, i16, i32   32-bit key: the value sign-extended to 32 bits, sign bit
 *                  flipped (key ^ 0x80000000 is the value).
 *   u64 / i64      64-bit key: the value / the value with its sign bit flipped.
 *   f32 / f64      32- / 64-bit key: add 0 (so -0.0 becomes +0.0), take the
 *                  bits u; if the sign bit is set the key is ~u, otherwise
 *                  u | sign.  Back: key & sign ? key ^ sign : ~key.
 *                  NaN has no key: it counts in `nan`, decided on the value.
 * A pass counts one digit: `bits` bits (1..PYAS_SELECT_MAX_BITS) at `shift`.
 * Table row of one output: 2^bits digit counts, then below, above, nan: the
 * histogram's row of 2^bits + 3 int64, zeroed by pyas_hist_reset(n_bins =
 * 2^bits).  With hi = key >> (shift + bits) (0 when the digit is the key's
 * first), an element adds 1 to slot (key >> shift) & (2^bits - 1) when hi ==
 * prefix[row], to `below` when hi < prefix[row], to `above` when hi >
 * prefix[row].  On every pass counts + below + above + nan is the row's
 * unmasked element count.  pyas_select_step then extends each row's prefix by
 * the digit that holds its rank; after the last digit (shift 0) prefix[row] is
 * the key of the row's rank-th smallest element. */
#define PYAS_SELECT_MAX_BITS 11
typedef struct {
    const uint64_t *prefix;  /* device, one per table row; NULL on the first pass (every prefix 0) */
    int32_t shift;           /* the digit's lowest bit; shift + bits <= the key's width */
    int32_t bits;            /* 1..PYAS_SELECT_MAX_BITS */
} pyas_select;

/* pyas_hist_axes with the digit rule (same argument checks, row mapping and
 * errors): with every dim in axes_mask the counts go through LDS into row 0 and
 * prefix[0] is the one prefix.  PYAS_EINVAL when select or table is NULL, bits
 * or shift is out of range, or prefix is NULL below the first digit. */
int pyas_select_axes(pyas_ctx *ctx, const pyas_batch *batch, const pyas_mask *mask,
                     const pyas_select *select, uint32_t axes_mask, const int64_t *out_offsets,
                     const int64_t *out_index, int64_t *table, void *stream);
/* Between passes, one wave per row (all pointers device): the running count
 * starts at the row's `below`, plus below_base[row] when below_base is not
 * NULL; the first digit j at which it exceeds rank[row] (zero-based, among the
 * row's non-NaN elements) gives prefix[row] = (prefix[row] << bits) | j.  A row
 * whose digit counts are all zero keeps its prefix.  The caller zeroes prefix
 * before the first pass. */
int pyas_select_step(pyas_ctx *ctx, const int64_t *table, int64_t n_rows, int32_t bits,
                     const int64_t *rank, uint64_t *prefix, const int64_t *below_base, void *stream);
/* One wave per row (device pointers): totals[2 row] = the sum of the row's
 * 2^bits + 3 slots (its unmasked elements, NaN included), totals[2 row + 1] =
 * its nan slot.  What a caller needs of a pass's table to set the ranks,
 * without copying the table. */
int pyas_select_totals(pyas_ctx *ctx, const int64_t *table, int64_t n_rows, int32_t bits,
                       int64_t *totals, void *stream);

/* Result formatting on the device: the last step of Active._from_storage
 * (active.py:591-630) applied to n combined partials (device), so that only
 * the result's values and mask cross PCIe (9-16 bytes per output instead of
 * the 32-byte partial).  `values` (device) receives
 *   PYAS_FORMAT_SUM : the sum in the variable dtype for floats (the partial's
 *                     f64 rounded, as `out` of that dtype stores it), int64
 *                     for signed and uint64 for unsigned ints;
 *   PYAS_FORMAT_MIN / PYAS_FORMAT_MAX: the value in the variable dtype;
 *   PYAS_FORMAT_MEAN: float64, bit-identical to np.ma's `out / n`
 *                     (active.py:630): masked where n == 0, where the
 *                     quotient is not finite, or where np.ma's safe-divide
 *                     domain |out| * finfo(float).tiny >= |n| holds; a
 *                     masked element holds 0.0 + f64(out) as np.ma leaves it.
 * mask (device) receives one byte per element (1 = masked); counts (device,
 * may be NULL) the partials' counts as int64 (the `n` of components mode). */
enum { PYAS_FORMAT_SUM = 0, PYAS_FORMAT_MIN = 1, PYAS_FORMAT_MAX = 2, PYAS_FORMAT_MEAN = 3 };
int pyas_format_partials(pyas_ctx *ctx, int32_t dtype, const pyas_partial *in, int64_t n,
                         int32_t method, void *values, uint8_t *mask, int64_t *counts,
                         void *stream);

/* Standalone HDF5/numcodecs byte un-shuffle (storage.py:121-122), device to
 * device; n_bytes % elementsize trailing bytes are copied through. */
int pyas_unshuffle(pyas_ctx *ctx, const void *src, void *dst, int64_t n_bytes,
                   int32_t elementsize, void *stream);

/* Batched un-shuffle of n_chunks whole chunks of chunk_bytes each, device to
 * device: chunk i from src + src_offsets[i] to dst + dst_offsets[i] (both
 * offset arrays in device memory); elementsize 2, 4 or 8 (PYAS_ENOTSUP
 * otherwise); trailing chunk_bytes % elementsize bytes are copied through.
 * Resident variables keep their chunks un-shuffled this way, so later
 * queries take the dense kernels (storage.py:121-122 once per chunk). */
int pyas_unshuffle_chunks(pyas_ctx *ctx, const void *src, const int64_t *src_offsets, void *dst,
                          const int64_t *dst_offsets, int64_t n_chunks, int64_t chunk_bytes,
                          int32_t elementsize, void *stream);

/* ---- zlib inflate (row f3) ------------------------------------------------- */
/* Per-stream outcome of pyas_inflate, mirroring zlib inflate()'s failures
 * (zlib.error from zlib.decompress in the reference, storage.py:119-120). */
typedef enum {
    PYAS_INFLATE_OK = 0,
    PYAS_INFLATE_BAD_HEADER = 1,    /* "incorrect header check" / bad method  */
    PYAS_INFLATE_NEED_DICT = 2,     /* preset dictionary (FDICT)              */
    PYAS_INFLATE_BAD_BLOCK = 3,     /* "invalid block type"                   */
    PYAS_INFLATE_BAD_STORED = 4,    /* "invalid stored block lengths"         */
    PYAS_INFLATE_BAD_CODE = 5,      /* invalid code lengths / tree            */
    PYAS_INFLATE_BAD_SYMBOL = 6,    /* invalid literal/length/distance code   */
    PYAS_INFLATE_BAD_DISTANCE = 7,  /* "invalid distance too far back"        */
    PYAS_INFLATE_TRUNCATED = 8,     /* "incomplete or truncated stream"       */
    PYAS_INFLATE_BAD_CHECKSUM = 9,  /* "incorrect data check" (Adler-32)      */
    PYAS_INFLATE_OVERFLOW = 10      /* output larger than dst_capacity        */
} pyas_inflate_status;

/* Inflate n independent zlib (RFC 1950) streams, device to device
 * (replaces numcodecs.Zlib.decode -> zlib.decompress at storage.py:119-120;
 * built by hdf2numcodec.py:34-35).  Stream c is src[src_offsets[c] ..
 * + src_sizes[c]) and inflates into dst[dst_offsets[c] .. + dst_capacity[c]);
 * out_sizes[c] receives the inflated length and status[c] a
 * pyas_inflate_status.  All arrays are device arrays.  Bytes after the
 * Adler-32 trailer are ignored, as zlib.decompress does.  A dst offset that is
 * 16-byte aligned gets 1 KiB coalesced writes. */
int pyas_inflate(pyas_ctx *ctx, const uint8_t *src, const int64_t *src_offsets,
                 const int64_t *src_sizes, int64_t n, uint8_t *dst,
                 const int64_t *dst_offsets, const int64_t *dst_capacity,
                 int64_t *out_sizes, int32_t *status, void *stream);

/* ---- host ingest (row f2) ------------------------------------------------ */
/* Positioned reads of n byte ranges of an open file straight into device
 * memory.  Replaces the reference's per-chunk open + read_block
 * (storage.py:51-53, :156-162) run on active.py:557's 30-thread pool.
 * Range i is file[file_offsets[i] .. + sizes[i]) and lands at
 * dst + dst_offsets[i] (dst: device).  `threads` reader threads pread(2)
 * into a ring of pinned staging slots; each filled slot is copied H2D on
 * `stream` while the next slots are read.  Returns once every copy is
 * enqueued on `stream`: work queued after it on that stream sees the data.
 * A read error or end of file before a range ends -> PYAS_EIO.  The offset
 * and size arrays are host arrays. */
int pyas_read_ranges(pyas_ctx *ctx, int fd, int64_t n, const int64_t *file_offsets,
                     const int64_t *sizes, void *dst, const int64_t *dst_offsets,
                     int32_t threads, void *stream);
/* pyas_read_ranges for zlib-compressed chunks inflated on the HOST: each
 * range is one zlib stream (storage.py:119-120 through numcodecs.Zlib,
 * hdf2numcodec.py:34-35) that the reader thread preads and inflates
 * straight into its pinned staging slot; the inflated out_bytes are copied
 * H2D to dst + dst_offsets[i].  status (host, n entries) receives a
 * pyas_inflate_status per stream (PYAS_INFLATE_OVERFLOW also for an output
 * shorter or longer than out_bytes); a failed stream's bytes in dst are
 * undefined and the caller raises (re-running zlib gives zlib's message).
 * Few streams inflate faster here than with pyas_inflate, whose per-stream
 * rate is one serial DEFLATE decoder; Active picks the side per query. */
int pyas_read_ranges_zlib(pyas_ctx *ctx, int fd, int64_t n, const int64_t *file_offsets,
                          const int64_t *sizes, void *dst, const int64_t *dst_offsets,
                          int64_t out_bytes, int32_t *status, int32_t threads, void *stream);
/* Staging ring of pyas_read_ranges: n_slots x slot_bytes of pinned host
 * memory (default 16 x 64 MiB; each slot is pinned on first use). */
int pyas_ctx_set_ingest_slots(pyas_ctx *ctx, int32_t n_slots, int64_t slot_bytes);

/* ---- per-chunk drop-in, coalesced across threads ------------------------- */
/* The reference's Active._from_storage calls reduce_chunk once per chunk from
 * a 30-thread pool (active.py:556-589 -> :765-776 -> storage.py:8-104), each
 * call opening the file and reading its chunk (storage.py:51-53,156-162).
 * pyas_coalesced_reduce is that per-chunk call, thread-safe and blocking: the
 * calling thread preads its chunk into a pinned ring shared by all callers,
 * and a dispatcher thread reduces every chunk whose read has completed in one
 * H2D copy, one zlib-inflate launch and one reduce launch per (layout, mask,
 * axes) group, then wakes the callers.  Same per-chunk results as
 * pyas_reduce_chunks / pyas_reduce_axes on that chunk. */
typedef struct {
    int32_t dtype;                     /* pyas_dtype */
    int32_t byteswap;                  /* 1: stored non-native (big-endian) */
    int32_t shuffle;                   /* fused HDF5 shuffle (== itemsize) or 0 */
    int32_t ndim;
    int64_t chunk_shape[PYAS_MAX_DIMS];
    int32_t zlib;                      /* 1: the file bytes are one zlib stream
                                          (hdf2numcodec.py:34-35, storage.py:119-120) */
    uint32_t axes_mask;                /* chunk dims reduced (all dims: one partial) */
    uint32_t tie_which;                /* NumPy's zero sign for min (1) / max (2): pyas_tie_chunks */
    pyas_tie_geom tie;
} pyas_chunk_desc;

typedef struct pyas_coalescer pyas_coalescer;

/* ring_bytes: pinned host ring + device mirror (0 = 256 MiB); max_batch:
 * most chunks per dispatch (0 = 4096).  Starts the dispatcher thread. */
int pyas_coalescer_create(pyas_ctx *ctx, int64_t ring_bytes, int32_t max_batch,
                          pyas_coalescer **out);
int pyas_coalescer_destroy(pyas_coalescer *c);
/* stats (int64[8]): batches dispatched, chunks reduced, largest batch,
 * dispatcher busy ns (launching), callers' file-read ns, callers'
 * wait-for-batch ns, device-queue ns (per batch: from its launch, or the
 * previous batch's completion if later, to its completion), requests
 * handed back to the per-call path */
int pyas_coalescer_stats(pyas_coalescer *c, int64_t *stats);
/* Reduce file `path` bytes [offset, offset + size) as one chunk described by
 * desc/mask (mask without vector tables), selection `sel` (host
 * [PYAS_MAX_DIMS*3] as in pyas_batch, NULL = whole chunk) with `pool`
 * (host, pool_len entries) for listed dims.  `out` (host) receives n_out
 * partials (n_out must equal the kept selected extents' product, 1 when
 * every dim is reduced).  info (host int64[3]): bytes read (or -errno if the
 * open failed), inflate status, inflated size.  Returns PYAS_OK, or
 * PYAS_EIO for an open/read failure, short read or failed/mis-sized inflate,
 * PYAS_ENOTSUP for what the coalescer does not take (vector mask tables, a
 * chunk larger than the ring, uncompressed size != chunk bytes): the caller
 * then runs the per-call path, which raises the reference's exact error. */
int pyas_coalesced_reduce(pyas_coalescer *c, const char *path, int64_t offset, int64_t size,
                          const pyas_chunk_desc *desc, const pyas_mask *mask,
                          const int32_t *sel, const int32_t *pool, int32_t pool_len,
                          int64_t n_out, pyas_partial *out, int64_t *info);

/* ---- measurement ---------------------------------------------------------- */
/* When enabled, the main reduce kernel of each pyas_reduce_chunks call is
 * bracketed by HIP events on the launch stream (up to max_launches calls). */
int pyas_timing_enable(pyas_ctx *ctx, int32_t max_launches);
/* Synchronises the recorded events; writes up to cap durations (ms). */
int pyas_timing_read(pyas_ctx *ctx, float *ms, int32_t cap, int32_t *n);

#ifdef __cplusplus
}
#endif
#endif /* PYAS_H */
