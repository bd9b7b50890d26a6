// pyas_hist.hip — binned counts behind Active.histogram (pyas_hist_axes of
// include/pyas.h).
//
// One pass over the same bytes a mean reads.  Every unmasked selected element
// converts to f64 as astype(float64) does and adds 1 to one slot of its
// output's table row: n_bins counts, then below, above, nan (all int64).
// Bin i holds e[i] <= x < e[i+1], the last bin also x == e[n].  Integers add in
// any order, so results are exact and bit-identical from run to run.
//
// Bin index: a guess int(x * scale - lo * scale) clamped to [0, n-1] (uniform
// edges; 0 otherwise), checked against e[i] and e[i+1].  A miss takes the slow
// path: NaN / below / above / last bin, then for uniform edges up to two steps
// of one bin, then a binary search.  Only the edge table decides, so any
// strictly increasing edges bin correctly whatever the guess was.
//
// k_hist_full : every dim reduced, n_bins <= kHistLdsBins.  A capped grid; each
//               workgroup walks a contiguous range of (chunk, tile) pairs and
//               counts into 32-bit LDS tables with ds atomics.  The table is
//               replicated `copies` times (slot-major, copy = thread % copies):
//               with 32 copies the 32 lanes an LDS pass serves hit 32 banks, so
//               a hot bin costs what a spread one does; a masked element adds
//               to a spare slot, so the add needs no branch.  The copies are summed
//               and added to the global int64 row (64-bit atomics, zero slots
//               skipped) at the workgroup's end, when the output row changes,
//               and before a copy could pass 2^32.  Whole chunks and one-run
//               selections stream 16-B loads, register double-buffered;
//               anything else walks per element.
// k_hist_axes : partial axes, and every n_bins above kHistLdsBins.  Walks per
//               element; one global 64-bit atomic add per unmasked element.
//               Innermost dim kept: a lane per output.  Innermost dim reduced:
//               `split` waves per output, equal slots of a wave added once.
// Both are templated on the dtype and shuffled-or-not only; byte order, mask
// rules and selection kind are run-time branches.
#include <hip/hip_runtime.h>

#include "pyas_hist_walk.hpp"   // the counting accumulators, hist_row, hist_flush; the runs and the walk

namespace pyas {

// largest i in [0, n-1] with e[i] <= x, given e[0] <= x < e[n]
__device__ __forceinline__ int hist_search(const double *e, int n, double x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
}

// The slot of x when the guess i (in [0, n-1]) missed.
__device__ __forceinline__ int hist_slot_slow(const double *e, int n, bool uniform, int i, double x) {
    if (x != x) return n + 2;
    if (x < e[0]) return n;
    if (x > e[n]) return n + 1;
    if (x >= e[n - 1]) return n - 1;          // the last bin is closed: x == e[n] too
    // e[0] <= x < e[n-1], so n >= 2 and every index below stays in [0, n-1]
    if (uniform) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (x < e[i]) --i;
            else if (x >= e[i + 1]) ++i;
        }
        if (e[i] <= x && x < e[i + 1]) return i;
    }
    return hist_search(e, n, x);
}

struct HistBins {
    const double *e;       // n + 1 edges
    int n;
    bool uniform;
    double scale, off;     // the guess: x * scale + off = (x - lo) * scale
    __device__ __forceinline__ void init(const HistArgs &a, const double *edges) {
        e = edges;
        n = a.n_bins;
        uniform = a.uniform != 0;
        scale = a.scale;
        off = -a.lo * a.scale;
        if (!(off == off) || !uniform) {   // no guess (or lo * scale overflowed): bin 0, then the search
            scale = 0.0;
            off = 0.0;
        }
    }
    // The slots of N values; ok[k]: x[k] is selected and unmasked (the other
    // slots are in [0, n-1] but mean nothing).  The guesses are checked inline;
    // the misses (rare) go one at a time through a single copy of the slow path.
    template <int N, typename T>
    __device__ __forceinline__ void slots(const T *x, const bool *ok, int *idx) const {
        bool hit[N], any = false;
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const double xd = (double)x[k];
            // the conversion saturates and gives 0 for NaN; whatever it gives, the index is clamped
            int i = (int)__builtin_fma(xd, scale, off);
            i = i < 0 ? 0 : i;
            i = i > n - 1 ? n - 1 : i;
            const double e0 = e[i], e1 = e[i + 1];
            idx[k] = i;
            hit[k] = e0 <= xd && xd < e1;
            any |= ok[k] && !hit[k];
        }
        if (__builtin_expect(any, 0)) {
            uint32_t miss = 0;
#pragma unroll
            for (int k = 0; k < N; ++k) miss |= (ok[k] && !hit[k]) ? 1u << k : 0u;
            while (miss != 0) {
                const int k = __builtin_ctz(miss);
                miss &= miss - 1;
                T xv = x[0];
                int iv = idx[0];
#pragma unroll
                for (int j = 1; j < N; ++j) {
                    xv = k == j ? x[j] : xv;
                    iv = k == j ? idx[j] : iv;
                }
                const int s = hist_slot_slow(e, n, uniform, iv, (double)xv);
#pragma unroll
                for (int j = 0; j < N; ++j) idx[j] = k == j ? s : idx[j];
            }
        }
    }
};

// the accumulators of pyas_hist_walk.hpp under the bin rule
using HistLds = CountLds<HistBins>;
using HistLane = CountLane<HistBins>;
using HistWave = CountWave<HistBins>;

// ---------------------------------------------------------------------------
// every dim reduced: workgroup g walks pairs [g P / G, (g + 1) P / G), pair =
// tile t of chunk c
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) PYAS_HIST_WAVES(T) void k_hist_full(HistArgs a) {
    extern __shared__ double s_hist[];   // n_bins + 1 edges, then (slots + 1 spare) * copies counts
    const ReduceArgs &r = a.r;
    const int n = a.n_bins, slots = n + 3, shift = a.shift;
    double *s_e = s_hist;
    uint32_t *s_tab = reinterpret_cast<uint32_t *>(s_hist + n + 1);
    for (int k = threadIdx.x; k <= n; k += kBlock) s_e[k] = a.edges[k];
    for (int k = threadIdx.x; k < ((slots + 1) << shift); k += kBlock) s_tab[k] = 0;
    __syncthreads();
    HistLds acc;
    acc.b.init(a, s_e);
    acc.tab = reinterpret_cast<uint8_t *>(s_tab + (threadIdx.x & ((1 << shift) - 1)));
    acc.sh = shift + 2;
    MaskT<T> mk;
    mk.init(r.mask);
    const bool tabs = r.tab.on[0] || r.tab.on[1];
    const int64_t p0 = (int64_t)blockIdx.x * a.n_pairs / gridDim.x;
    const int64_t p1 = ((int64_t)blockIdx.x + 1) * a.n_pairs / gridDim.x;
    int64_t cur_row = 0;
    uint64_t pending = 0;   // elements handed to the LDS table since its last flush
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t c = p / a.bpc, t = p % a.bpc;
        const uint8_t *base = r.data + r.offsets[c];
        Sel s;
        load_sel(s, r.sel, c, r.ndim, r.shape);
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
        if (e0 >= e1) continue;
        const int64_t row = hist_row(a.out_offsets, a.out_index, c, 0);
        // a copy's count is at most `pending` (< 2^31 per pair): flush before it could wrap
        if (pending && (row != cur_row || pending + (uint64_t)(e1 - e0) > 0xFFFFFFFFull)) {
            hist_flush(s_tab, slots, shift, a.table + cur_row * slots);
            pending = 0;
        }
        cur_row = row;
        pending += (uint64_t)(e1 - e0);
        if (contig) {
            const int mode = mask_mode(a.masked, r.mask.flags);
            if (a.bswap) stat_run<T, SHUF, true>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
            else stat_run<T, SHUF, false>(mode, base, r.chunk_elems, m0 + e0, m0 + e1, acc, mk);
        } else if (e0 + threadIdx.x < e1) {
            const uint32_t all = (1u << r.ndim) - 1u;
            RadixCounter rc;
            rc.init(s, r.ndim, all, (uint64_t)(e0 + threadIdx.x), (uint64_t)kBlock);
            const Decomp zero{0, {0, 0}};
            stat_walk<T, SHUF>(r, base, s, all, zero, rc, e0 + threadIdx.x, e1, kBlock, a.bswap, mk, acc);
        }
    }
    if (pending) hist_flush(s_tab, slots, shift, a.table + cur_row * slots);
}

// ---------------------------------------------------------------------------
// partial axes and the generic form: global atomics into
// table[row(c, o) * slots + slot], o in C order over the kept selected dims
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_hist_axes(HistArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    const int64_t slots = (int64_t)a.n_bins + 3;
    // the edges from LDS when they fit
    __shared__ double s_e[kHistLdsBins + 1];
    const double *e = a.edges;
    if (a.n_bins <= kHistLdsBins) {   // uniform
        for (int k = threadIdx.x; k <= a.n_bins; k += kBlock) s_e[k] = a.edges[k];
        __syncthreads();
        e = s_e;
    }
    HistBins bins;
    bins.init(a, e);
    Sel s;
    load_sel(s, r.sel, c, r.ndim, r.shape);
    MaskT<T> mk;
    mk.init(r.mask);
    const uint32_t red = a.axes, keep = ~a.axes & ((1u << r.ndim) - 1u);
    int64_t n_keep, n_red;
    axes_extents(s, r.ndim, red, n_keep, n_red);
    if (n_red <= 0) return;
    if (!a.row) {   // a lane per output
        for (int64_t o = b * kBlock + threadIdx.x; o < n_keep; o += a.bpc * kBlock) {
            Decomp bo{0, {0, 0}};
            decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
            RadixCounter rc;
            rc.init(s, r.ndim, red, 0, 1);
            const HistLane acc{bins, a.table + hist_row(a.out_offsets, a.out_index, c, o) * slots};
            stat_walk<T, SHUF>(r, base, s, red, bo, rc, 0, n_red, 1, a.bswap, mk, acc);
        }
    } else {        // `split` waves per output: wave part takes positions part * 64 + lane, + split * 64, ...
        constexpr int kWaves = kBlock / kWave;
        const int lane = threadIdx.x & (kWave - 1);
        const int64_t split = a.split;
        for (int64_t u = b * kWaves + threadIdx.x / kWave; u < n_keep * split; u += a.bpc * kWaves) {
            const int64_t o = u / split, q0 = (u % split) * kWave + lane;
            if (q0 < n_red) {
                Decomp bo{0, {0, 0}};
                decompose(s, r.pool, r.cstride, r.tab, r.ndim, keep, o, bo);
                RadixCounter rc;
                rc.init(s, r.ndim, red, (uint64_t)q0, (uint64_t)(split * kWave));
                const HistWave acc{bins, a.table + hist_row(a.out_offsets, a.out_index, c, o) * slots};
                stat_walk<T, SHUF>(r, base, s, red, bo, rc, q0, n_red, split * kWave, a.bswap, mk, acc);
            }
        }
    }
}

hipError_t launch_hist_full(int dtype, const HistArgs &a, bool shuf, int64_t grid, size_t lds, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_hist_full), a, shuf, grid, lds, st)
}

hipError_t launch_hist_axes(int dtype, const HistArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_hist_axes), a, shuf, grid, 0, st)
}

}  // namespace pyas
