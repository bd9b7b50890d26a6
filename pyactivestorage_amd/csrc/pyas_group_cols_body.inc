// pyas_group_cols_body.inc — the body of k_group_cols and k_group_cols_partial
// (pyas_grouped.hip), included inside each kernel after `using A = <accumulator>;`
// with T, SHUF and the kernel argument `a` in scope.  It is text, not a function:
// called as a function template the MomAcc instance compiles to other registers
// (gfx950: 6 fewer SGPRs for every dtype, 163 -> 137 VGPRs for f64), and
// k_group_cols is held to the resources it was measured with.
    using R = typename GrRec<A>::R;
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
    GrLane<A> ln;
#pragma unroll
    for (int k = 0; k < V; ++k) ln.acc[k].init();
    ln.cur = -1;
    ln.hunt = true;
    R *out = static_cast<R *>(a.out) + fidx;   // the lane's 4 outputs are adjacent: the innermost dim's output stride is 1
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
