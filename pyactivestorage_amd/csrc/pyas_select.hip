// pyas_select.hip — the exact k-th smallest element behind Active.quantile
// (pyas_select_axes and pyas_select_step of include/pyas.h): a radix select,
// most significant digit first, over the order-preserving unsigned key of
// every unmasked selected element.
//
// A pass is a histogram of one digit: table rows of 2^bits + 3 int64 (digit
// counts, then below, above, nan: the histogram's row).  With hi = the key's
// bits above the digit, an element counts in its digit's slot when hi equals
// its output's prefix (the digits found so far), in `below` when hi is less,
// in `above` when it is more; NaN counts in `nan` and has no key.  Counts are
// integers, so every pass is exact and the same from run to run.
//
// k_qsel_full : every dim reduced.  k_hist_full with the digit rule: replicated
//               32-bit LDS tables, a capped grid, one flush per workgroup (and
//               before a copy could pass 2^32).  No edges in LDS; the one prefix
//               is read once per workgroup into a scalar register.
// k_qsel_axes : partial axes.  k_hist_axes with the digit rule: global 64-bit
//               atomics, a lane per output or `split` waves per output; the
//               row's prefix is read once per output.
// k_qsel_step : a wave per row; the first digit whose running count (from
//               `below`) exceeds the row's rank extends its prefix.
// k_qsel_totals: a wave per row; the row's sum (the unmasked elements) and its
//               nan slot, so that a table never travels to the host.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pyas_hist_walk.hpp"   // the counting accumulators, hist_row, hist_flush; the runs and the walk

namespace pyas {

// The key (include/pyas.h): unsigned, in the order of the values; 32 bits for
// 1-, 2- and 4-byte types, 64 for 8-byte ones.
template <typename T>
using qsel_key_t = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;

template <typename T>
__device__ __forceinline__ qsel_key_t<T> qsel_key(T x) {
    using K = qsel_key_t<T>;
    constexpr K sign = (K)1 << (sizeof(K) * 8 - 1);
    if constexpr (std::is_floating_point_v<T>) {
        const T z = x + (T)0;   // -0.0 -> +0.0
        K u;
        __builtin_memcpy(&u, &z, sizeof(K));
        return (u & sign) ? ~u : (u | sign);
    } else if constexpr (std::is_signed_v<T>) {
        using S = std::conditional_t<sizeof(T) == 8, int64_t, int32_t>;
        return (K)(S)x ^ sign;
    } else {
        return (K)x;
    }
}

// The digit rule of one output in one pass.
template <typename T>
struct QselDigits {
    using K = qsel_key_t<T>;
    K prefix;              // the key's bits above the digit, found by the earlier passes
    K mask;                // 2^bits - 1
    int n;                 // 2^bits
    int shift;             // the digit's lowest bit
    int top;               // shift + bits, as a shift count: 0 when nothing is above the digit
    bool first;            //   (then hi == prefix == 0 for every key: a shift by the key's width is not one)
    __device__ __forceinline__ void init(int32_t shift_, int32_t bits, uint64_t prefix_) {
        constexpr int W = (int)sizeof(K) * 8;
        shift = shift_;
        n = 1 << bits;
        mask = (K)(n - 1);
        first = shift_ + bits >= W;
        top = first ? 0 : shift_ + bits;
        prefix = first ? (K)0 : (K)prefix_;
    }
    template <int N>
    __device__ __forceinline__ void slots(const T *x, const bool *ok, int *idx) const {
#pragma unroll
        for (int k = 0; k < N; ++k) {
            const K key = qsel_key(x[k]);
            const K hi = first ? (K)0 : (K)(key >> top);
            int s = (int)((key >> shift) & mask);
            s = hi < prefix ? n : s;
            s = hi > prefix ? n + 1 : s;
            if constexpr (std::is_floating_point_v<T>) s = x[k] != x[k] ? n + 2 : s;   // decided on the value, not its key
            idx[k] = s;
        }
    }
};

template <typename T>
using QselLds = CountLds<QselDigits<T>>;
template <typename T>
using QselLane = CountLane<QselDigits<T>>;
template <typename T>
using QselWave = CountWave<QselDigits<T>>;

// ---------------------------------------------------------------------------
// every dim reduced: workgroup g walks pairs [g P / G, (g + 1) P / G), pair =
// tile t of chunk c (k_hist_full)
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) PYAS_HIST_WAVES(T) void k_qsel_full(QselArgs a) {
    extern __shared__ uint32_t s_qsel[];   // (slots + 1 spare) * copies counts
    const ReduceArgs &r = a.r;
    const int slots = (1 << a.bits) + 3, shift = a.shift_copies;
    for (int k = threadIdx.x; k < ((slots + 1) << shift); k += kBlock) s_qsel[k] = 0;
    __syncthreads();
    QselLds<T> acc;
    acc.b.init(a.shift, a.bits, a.prefix ? a.prefix[0] : 0ull);   // one row: one prefix
    acc.tab = reinterpret_cast<uint8_t *>(s_qsel + (threadIdx.x & ((1 << shift) - 1)));
    acc.sh = shift + 2;
    MaskT<T> mk;
    mk.init(r.mask);
    const bool tabs = r.tab.on[0] || r.tab.on[1];
    const int64_t p0 = (int64_t)blockIdx.x * a.n_pairs / gridDim.x;
    const int64_t p1 = ((int64_t)blockIdx.x + 1) * a.n_pairs / gridDim.x;
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
        // a copy's count is at most `pending` (< 2^31 per pair): flush before it could wrap
        if (pending && pending + (uint64_t)(e1 - e0) > 0xFFFFFFFFull) {
            hist_flush(s_qsel, slots, shift, a.table);
            pending = 0;
        }
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
    if (pending) hist_flush(s_qsel, slots, shift, a.table);
}

// ---------------------------------------------------------------------------
// partial axes: global atomics into table[row(c, o) * slots + slot], o in C
// order over the kept selected dims (k_hist_axes)
// ---------------------------------------------------------------------------
template <typename T, bool SHUF>
__global__ __launch_bounds__(kBlock) void k_qsel_axes(QselArgs a) {
    const ReduceArgs &r = a.r;
    const int64_t c = (int64_t)blockIdx.x / a.bpc, b = (int64_t)blockIdx.x % a.bpc;
    const uint8_t *base = r.data + r.offsets[c];
    const int64_t slots = ((int64_t)1 << a.bits) + 3;
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
            const int64_t row = hist_row(a.out_offsets, a.out_index, c, o);
            QselLane<T> acc;
            acc.b.init(a.shift, a.bits, a.prefix ? a.prefix[row] : 0ull);
            acc.row = a.table + row * slots;
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
                const int64_t row = hist_row(a.out_offsets, a.out_index, c, o);
                QselWave<T> acc;
                acc.b.init(a.shift, a.bits, a.prefix ? a.prefix[row] : 0ull);
                acc.row = a.table + row * slots;
                stat_walk<T, SHUF>(r, base, s, red, bo, rc, q0, n_red, split * kWave, a.bswap, mk, acc);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// between passes: a wave per row.  The running count starts at the row's
// `below` (plus below_base[row]); the first digit at which it exceeds
// rank[row] is shifted into prefix[row].  A row with nothing to select from
// (n - nan == 0) keeps prefix 0; a rank past the row's last element takes the
// last digit that holds one.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_qsel_step(const unsigned long long *table, int64_t n_rows, int32_t bits,
                                                      const int64_t *rank, unsigned long long *prefix,
                                                      const int64_t *below_base) {
    constexpr int kWaves = kBlock / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
    if (row >= n_rows) return;   // whole waves leave: the shuffles below see full ones
    const int n = 1 << bits;
    const unsigned long long *t = table + row * (int64_t)(n + 3);
    const unsigned long long want = (unsigned long long)rank[row];
    unsigned long long run = t[n] + (below_base ? (unsigned long long)below_base[row] : 0ull);
    int found = -1, last = -1;
    for (int j0 = 0; j0 < n && found < 0; j0 += kWave) {
        const int j = j0 + lane;
        const unsigned long long cnt = j < n ? t[j] : 0ull;
        unsigned long long inc = cnt;   // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const unsigned long long up = __shfl_up(inc, d);
            if (lane >= d) inc += up;
        }
        const uint64_t over = __ballot(run + inc > want);
        const uint64_t any = __ballot(cnt != 0);
        if (over) found = j0 + __builtin_ctzll(over);
        if (any) last = j0 + 63 - __builtin_clzll(any);
        run += __shfl(inc, kWave - 1);
    }
    if (found < 0) found = last;
    if (found < 0) return;       // an empty row
    if (lane == 0) prefix[row] = (prefix[row] << bits) | (unsigned long long)found;
}

// totals[2 row] = the sum of the row's slots, totals[2 row + 1] = its nan slot
__global__ __launch_bounds__(kBlock) void k_qsel_totals(const unsigned long long *table, int64_t n_rows, int32_t bits,
                                                        int64_t *totals) {
    constexpr int kWaves = kBlock / kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t row = (int64_t)blockIdx.x * kWaves + threadIdx.x / kWave;
    if (row >= n_rows) return;   // whole waves leave
    const int slots = (1 << bits) + 3;
    const unsigned long long *t = table + row * (int64_t)slots;
    unsigned long long sum = 0;
    for (int j = lane; j < slots; j += kWave) sum += t[j];
#pragma unroll
    for (int d = kWave / 2; d > 0; d >>= 1) sum += __shfl_xor(sum, d);
    if (lane == 0) {
        totals[2 * row] = (int64_t)sum;
        totals[2 * row + 1] = (int64_t)t[slots - 1];
    }
}

hipError_t launch_qsel_full(int dtype, const QselArgs &a, bool shuf, int64_t grid, size_t lds, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_qsel_full), a, shuf, grid, lds, st)
}

hipError_t launch_qsel_axes(int dtype, const QselArgs &a, bool shuf, int64_t grid, hipStream_t st) {
    PYAS_DISPATCH_DTYPE(launch_shuf, PYAS_SHUF_KERNEL(k_qsel_axes), a, shuf, grid, 0, st)
}

hipError_t launch_qsel_step(const unsigned long long *table, int64_t n_rows, int32_t bits, const int64_t *rank,
                            unsigned long long *prefix, const int64_t *below_base, hipStream_t st) {
    constexpr int64_t kWaves = kBlock / kWave;
    const int64_t grid = (n_rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_qsel_step, dim3((unsigned)grid), dim3(kBlock), 0, st, table, n_rows, bits, rank, prefix,
                       below_base);
    return hipGetLastError();
}

hipError_t launch_qsel_totals(const unsigned long long *table, int64_t n_rows, int32_t bits, int64_t *totals,
                              hipStream_t st) {
    constexpr int64_t kWaves = kBlock / kWave;
    const int64_t grid = (n_rows + kWaves - 1) / kWaves;
    hipLaunchKernelGGL(k_qsel_totals, dim3((unsigned)grid), dim3(kBlock), 0, st, table, n_rows, bits, totals);
    return hipGetLastError();
}

}  // namespace pyas
