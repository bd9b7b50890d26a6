// pyas_rolling.hpp — the running-window record (pyas_roll of include/pyas.h):
// its merge and the accumulator that walks one sequence position after
// position.  Plain C++ over pyas.h alone, so that a host program can hold both
// to a brute-force window scan; pyas_rolling.hip compiles them for the device.
//
// Every array is indexed by constants once the loops are unrolled (the window
// w only predicates), so on the device the record and the accumulator stay in
// registers.
#pragma once

#include <stdint.h>

#include "pyas.h"

#ifdef __HIPCC__
#define PYAS_ROLL_FN __device__ __forceinline__
#define PYAS_ROLL_UNROLL _Pragma("unroll")
#else
#define PYAS_ROLL_FN inline
#define PYAS_ROLL_UNROLL
#endif

namespace pyas {

constexpr int kRollH = PYAS_ROLL_MAX_WINDOW - 1;   // elements a record keeps at either end, at most

// Does the later candidate c replace the holder?  Strictly better only (the
// first among equals stays, -0.0 == +0.0), the first NaN wins and stays.
PYAS_ROLL_FN bool roll_beats(double c, double best, bool has, bool mn) {
    return !has || (best == best && (c != c || (mn ? c < best : c > best)));
}

struct RollMerge {
    // a's positions, then b's
    static PYAS_ROLL_FN pyas_roll merged(const pyas_roll &a, const pyas_roll &b) {
        constexpr int H = kRollH;
        const int w = a.window > b.window ? a.window : b.window;   // 0: both neutral
        const int h = w > 0 ? w - 1 : 0;
        const bool mn = (a.which | b.which) != 0;
        const int ta = a.len < h ? a.len : h, hb = b.len < h ? b.len : h;   // a's tail, b's head
        const uint32_t hmask = (1u << h) - 1u;
        pyas_roll r;
        double best = a.best;
        int32_t pos = a.position, nw = a.n_windows;
        // the windows across the seam, in sequence order: m elements of a's end, w - m of b's start
        PYAS_ROLL_UNROLL
        for (int m = H; m >= 1; --m) {
            if (m <= h) {
                const uint32_t tneed = (1u << m) - 1u, hneed = (1u << (w - m)) - 1u;
                const bool valid = (a.tail_ok & tneed) == tneed && (b.head_ok & hneed) == hneed;
                double s = a.tail[m - 1];
                PYAS_ROLL_UNROLL
                for (int j = m - 2; j >= 0; --j) s += a.tail[j];
                PYAS_ROLL_UNROLL
                for (int j = 0; j < H; ++j)
                    if (j < w - m) s += b.head[j];
                const bool take = valid && roll_beats(s, best, nw > 0, mn);
                best = take ? s : best;
                pos = take ? a.len - m : pos;
                nw += valid ? 1 : 0;
            }
        }
        {
            const bool take = b.n_windows > 0 && roll_beats(b.best, best, nw > 0, mn);
            best = take ? b.best : best;
            pos = take ? a.len + b.position : pos;
            nw += b.n_windows;
        }
        r.best = best;
        r.position = pos;
        r.n_windows = nw;
        r.n = a.n + b.n;
        r.len = a.len + b.len;
        r.window = (uint8_t)w;
        r.which = mn ? 1 : 0;
        r.reserved = 0;
        // the head grows only while a is shorter than h; the tail likewise from the end
        PYAS_ROLL_UNROLL
        for (int j = 0; j < H; ++j) {
            r.head[j] = a.head[j];
            r.tail[j] = b.tail[j];
        }
        PYAS_ROLL_UNROLL
        for (int t = 0; t < H; ++t) {
            if (ta == t) {
                PYAS_ROLL_UNROLL
                for (int j = t; j < H; ++j) r.head[j] = j < h ? b.head[j - t] : 0.0;
            }
            if (hb == t) {
                PYAS_ROLL_UNROLL
                for (int j = t; j < H; ++j) r.tail[j] = j < h ? a.tail[j - t] : 0.0;
            }
        }
        r.head_ok = (uint8_t)(((uint32_t)a.head_ok | ((uint32_t)b.head_ok << ta)) & hmask);
        r.tail_ok = (uint8_t)(((uint32_t)b.tail_ok | ((uint32_t)a.tail_ok << hb)) & hmask);
        return r;
    }
};

// The windows of one sequence, position after position.  T: the element type;
// P: the type the previous elements are held in: T itself for the types of up
// to 4 bytes, double for the 8-byte ones (pyas_rolling.hip; the sum reads
// float64(x) either way).
template <typename T, typename P>
struct RollAcc {
    P prev[kRollH];       // prev[i]: the element i + 1 positions back (0 when none), all 7 kept, masked ones too
    double best;
    int32_t position, n_windows, n, len;
    uint32_t ok;          // bit i: prev[i] exists and is unmasked
    uint32_t hok;         // head_ok so far

    PYAS_ROLL_FN void init() {
        PYAS_ROLL_UNROLL
        for (int i = 0; i < kRollH; ++i) prev[i] = (P)0;
        best = 0.0;
        position = 0;
        n_windows = 0;
        n = 0;
        len = 0;
        ok = 0;
        hok = 0;
    }
    // Before add(), while len < w - 1: the position is part of the head, which
    // goes straight to the record in memory (slot len), so that only the
    // shift register stays in registers.
    PYAS_ROLL_FN void head_slot(pyas_roll *out, T v, bool um) {
        out->head[len] = um ? (double)v : 0.0;
        hok |= (um ? 1u : 0u) << len;
    }
    // An element outside the window adds -0.0: -0.0 + x and x + -0.0 are x bit
    // for bit for every x, so the sum over all 7 slots is the window's own
    // chain of additions and no branch depends on w.  The price: every window
    // pays the 7 selects and 8 additions of a window of 8.
    // one position: its element and whether it is unmasked
    PYAS_ROLL_FN void add(T v, bool um, int w, bool mn) {
        const int h = w - 1;
        const uint32_t okc = ((ok << 1) | (um ? 1u : 0u)) & 0xffu, need = (1u << w) - 1u;
        const bool valid = (okc & need) == need;
        // the window that ends here, oldest element first
        double s = -0.0;
        PYAS_ROLL_UNROLL
        for (int j = kRollH - 1; j >= 0; --j) s += j < h ? (double)prev[j] : -0.0;
        s += (double)v;
        len += 1;
        const bool take = valid && roll_beats(s, best, n_windows > 0, mn);
        best = take ? s : best;
        position = take ? len - w : position;
        n_windows += valid ? 1 : 0;
        n += um ? 1 : 0;
        PYAS_ROLL_UNROLL
        for (int j = kRollH - 1; j >= 1; --j) prev[j] = prev[j - 1];
        prev[0] = (P)v;
        ok = okc;
    }
    PYAS_ROLL_FN void finish(pyas_roll *out, int w, bool mn) const {
        const int h = w - 1;
        PYAS_ROLL_UNROLL
        for (int j = 0; j < kRollH; ++j)
            if (j >= len || j >= h) out->head[j] = 0.0;   // the slots head_slot() did not write
        out->head_ok = (uint8_t)hok;
        out->best = best;
        out->position = position;
        out->n_windows = n_windows;
        out->n = n;
        out->len = len;
        out->window = (uint8_t)w;
        out->which = mn ? 1 : 0;
        out->tail_ok = (uint8_t)(ok & ((1u << h) - 1u));
        out->reserved = 0;
        PYAS_ROLL_UNROLL
        for (int k = 0; k < kRollH; ++k) out->tail[k] = (k < h && ((ok >> k) & 1u)) ? (double)prev[k] : 0.0;
    }
};

}  // namespace pyas
