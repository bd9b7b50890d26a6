"""Parity assertions between the HIP path and the oracle (test helper)."""
import math

import numpy as np


def shuffle_bytes(arr: np.ndarray, es: int) -> bytes:
    """HDF5/numcodecs shuffle *encode* (inverse of the decode under test)."""
    raw = np.frombuffer(arr.tobytes(), dtype=np.uint8)
    n = raw.size // es
    return raw[: n * es].reshape(n, es).T.reshape(-1).tobytes() + raw[n * es:].tobytes()


# float32 sums/means: NumPy sums float32 pairwise in float32, the GPU in
# float64 and rounds once; both are within a few ulp of the exact value, so we
# allow 1e-6 relative (north_star's bound) or, where the sum cancels, 4e-7 of
# the sum of |x| (NumPy pairwise error bound for these sizes).  float64
# results take sum_bound() below, and never more than this rule.
REL_TOL = 1e-6
ABS_FRAC = 4e-7

U64 = 2.0 ** -53                       # unit roundoff of float64
U32 = 2.0 ** -24                       # unit roundoff of float32
GAMMA3 = 3 * U32 / (1 - 3 * U32)       # three f32 roundings (Higham's gamma_3)
MEAN_ROUNDINGS = 1                     # k_format and Active._format: one f64 division
# The rules some tests used before sum_bound, as (rtol, atol) of
# ``atol + rtol |want|``: kept only as caps, a tolerance is min(cap, bound).
CAP_PARTIAL = (1e-6, 1e-3)             # raw per-chunk partial sums
CAP_FOLD_MEAN = (1e-5, 1e-4)           # Active means in test_gpu_axes_fold


def sum_bound(dtype, n, abs_sum, kind="sum", ref="exact", mean_abs=None, extended=False):
    """Largest |got - reference| a correct kernel can show for one output
    that reduces ``n`` unmasked values whose sum of magnitudes is ``abs_sum``.

    Derivation (u = 2**-53).  Any order or tree of n f64 additions is within
    (n - 1) u sum|x| of the exact sum, to first order (Higham, Accuracy and
    Stability of Numerical Algorithms, eq. 4.4); the exactly rounded
    reference (``math.fsum``) is within u |s| <= u sum|x| of it.  With the
    second-order terms rounded up:

      float64 data, or any path whose accumulator is f64 throughout (an
      integer mean), against the exact sum (``ref="exact"``):
          (n + 2) u sum|x|
      against NumPy's result (``ref="numpy"``, e.g. the golden files), whose
      own order error is another (n - 1) u sum|x| plus its final rounding:
          (2n + 2) u sum|x|
      a mean (``kind="mean"``): the sum's bound over n, plus k u |mean| for
      the k roundings of the kernel's own mean.  ``k_format`` computes
      ``(double)sum / (double)count`` and ``Active._format`` ``out / n`` in
      f64: one division each, k = MEAN_ROUNDINGS = 1 (the cast of an f64 sum
      to the f64 variable dtype is exact).  One more u |mean| for the
      reference's own division (exact sum / n rounded to f64, or NumPy's).
      ``mean_abs`` is |mean| (default sum|x| / n, its upper bound).
      float32 data, raw f64 partials (``partials["sum"]`` before any rounding
      to the variable dtype): ``TileAcc::add_group`` adds groups of at most
      four f32 values into an f32 zero (the first addition is exact: three
      f32 roundings per group, each element's error at most gamma_3 |x|),
      then the group sums in f64:
          gamma_3 sum|x| + (n + 2) u sum|x|,  gamma_3 = 3 u32 / (1 - 3 u32)
      ``extended``: the reference was summed in ``np.longdouble`` (64-bit
      mantissa) instead of exactly: n 2**-64 sum|x| more.

    Where sum|x| is not finite (NaN or infinity among the values), or n is 0,
    the bound is 0: only equality or a matching NaN passes, never an infinite
    tolerance."""
    dt = np.dtype(dtype)
    n = np.asarray(n, dtype=np.float64)
    s = np.asarray(abs_sum, dtype=np.float64)
    if ref not in ("exact", "numpy"):
        raise ValueError(ref)
    if kind not in ("sum", "mean"):
        raise ValueError(kind)
    order = (n + 2) if ref == "exact" else (2 * n + 2)
    with np.errstate(all="ignore"):
        b = order * U64 * s
        if dt.kind == "f" and dt.itemsize == 4:
            b = b + GAMMA3 * s
        elif dt.kind == "f" and dt.itemsize != 8:
            raise TypeError(f"no derived bound for {dt}")
        if extended:
            b = b + n * 2.0 ** -64 * s
        if kind == "mean":
            cnt = np.maximum(n, 1)
            m = s / cnt if mean_abs is None else np.abs(np.asarray(mean_abs, dtype=np.float64))
            b = b / cnt + (MEAN_ROUNDINGS + 1) * U64 * m
        b = np.where(np.isfinite(b) & np.isfinite(s) & (n > 0), b, 0.0)
    return b


def exact_reference(vals, axis=None, extended=False):
    """Per output (C order over the kept dims, flattened): the exactly
    rounded sum (``math.fsum``), sum|x| and n of the unmasked values of
    ``vals`` (array or MaskedArray), taken from its float64 copy (exact for
    every float and for integers below 2**53).  A row holding NaN or an
    infinity gets NumPy's own sum (NaN / inf) and a non-finite sum|x|.
    ``extended``: sum in ``np.longdouble`` instead of the per-output loop
    (add ``extended=True`` to sum_bound then); refused unless long double
    carries at least 63 mantissa bits."""
    m = np.ma.getmaskarray(vals)
    v = np.ma.getdata(vals).astype(np.float64)
    nd = v.ndim
    if axis is None:
        axis = tuple(range(nd))
    axis = tuple(sorted(a % nd for a in ((axis,) if np.isscalar(axis) else axis)))
    kept = [d for d in range(nd) if d not in axis]
    perm = kept + list(axis)
    n_out = int(np.prod([v.shape[d] for d in kept], dtype=np.int64))
    v2 = np.transpose(v, perm).reshape(n_out, -1)
    ok = ~np.transpose(m, perm).reshape(n_out, -1)
    z = np.where(ok, v2, 0.0)
    with np.errstate(all="ignore"):
        out = {"n": ok.sum(axis=1).astype(np.int64), "abs_sum": np.abs(z).sum(axis=1)}
        if extended:
            assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is no wider than float64 here"
            out["exact"] = z.astype(np.longdouble).sum(axis=1).astype(np.float64)
        else:
            ex = np.empty(n_out, dtype=np.float64)
            for i in range(n_out):
                row = z[i]
                ex[i] = math.fsum(row) if np.isfinite(out["abs_sum"][i]) else row.sum()
            out["exact"] = ex
    return out


def error_ratio(got, want, bound):
    """|got - want| / bound per element; 0 where equal or both NaN, inf where
    they differ and the bound is 0."""
    g = np.asarray(got, dtype=np.float64)
    w = np.asarray(want, dtype=np.float64)
    b = np.broadcast_to(np.asarray(bound, dtype=np.float64), w.shape)
    with np.errstate(all="ignore"):
        same = (np.isnan(g) & np.isnan(w)) | (g == w)
        err = np.abs(g - w)
        r = np.where(same, 0.0, np.where((b > 0) & np.isfinite(err), err / np.where(b > 0, b, 1.0), np.inf))
    return r


def assert_within(got, want, bound, what="", old=None):
    """Equal, both NaN, or |got - want| <= bound, element by element; with
    ``old`` (a tolerance array, an earlier rule) the smaller of the two.
    Returns the worst |got - want| / bound (for reports)."""
    b = np.asarray(bound, dtype=np.float64)
    if old is not None:
        with np.errstate(invalid="ignore"):
            b = np.where(np.isfinite(old), np.minimum(b, old), b)
    r = error_ratio(got, want, b)
    bad = ~(r <= 1.0)
    assert not bad.any(), (f"{what}: values {np.asarray(got)[bad]} != {np.asarray(want)[bad]} "
                           f"(bound {np.broadcast_to(b, r.shape)[bad]}, error/bound {r[bad]})")
    return float(r.max()) if r.size else 0.0


def assert_same(want, got, kind=None, data_abs_sum=None, what="", n=None, data_dtype=None):
    """Reference result vs GPU result: same container, dtype, shape, mask;
    values bit-exact except float sums/means.  Sums and means of float32
    data (np.ma.mean of f32 is a float64 result of an f32 sum): REL_TOL /
    ABS_FRAC.  float64 results of f64 data, and integer means: sum_bound
    against NumPy's result, and never more than the float32 rule.  A float64
    result needs ``data_dtype``, and with f64 or integer data also
    ``data_abs_sum`` and ``n`` (the unmasked values per output): it is an
    error to compare one without them."""
    assert type(got) is type(want), f"{what}: type {type(got)} != {type(want)}"
    assert got.dtype == want.dtype, f"{what}: dtype {got.dtype} != {want.dtype}"
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    keep = np.ones(want.shape, dtype=bool)
    if isinstance(want, np.ma.MaskedArray):
        wm, gm = np.ma.getmask(want), np.ma.getmask(got)
        assert (wm is np.ma.nomask) == (gm is np.ma.nomask), f"{what}: nomask mismatch {wm!r} {gm!r}"
        wma, gma = np.ma.getmaskarray(want), np.ma.getmaskarray(got)
        assert np.array_equal(wma, gma), f"{what}: mask {gma} != {wma}"
        keep = ~wma
    wd = np.asarray(np.ma.getdata(want))[keep]
    gd = np.asarray(np.ma.getdata(got))[keep]
    if wd.dtype.kind == "f" and kind in ("sum", "mean", None):
        w64, g64 = wd.astype(np.float64), gd.astype(np.float64)
        tol = REL_TOL * np.abs(w64)
        s = None
        if data_abs_sum is not None:
            s = np.broadcast_to(np.asarray(data_abs_sum, dtype=np.float64), want.shape)[keep]
            with np.errstate(invalid="ignore"):
                tol = np.maximum(tol, ABS_FRAC * s)
        if wd.dtype.itemsize == 8 and data_dtype is None:
            raise TypeError(f"{what}: a float64 sum or mean needs data_dtype (f64 and integer data "
                            "are compared with sum_bound())")
        if wd.dtype.itemsize == 8 and not (np.dtype(data_dtype).kind == "f" and np.dtype(data_dtype).itemsize < 8):
            if kind is None or s is None or n is None:
                raise TypeError(f"{what}: a float64 sum or mean is compared with sum_bound(): "
                                "pass kind, data_abs_sum and n")
            cnt = np.broadcast_to(np.asarray(n, dtype=np.float64), want.shape)[keep]
            b = sum_bound(np.float64, cnt, s, kind, ref="numpy", mean_abs=w64)
            with np.errstate(invalid="ignore"):
                tol = np.where(np.isfinite(tol), np.minimum(tol, b), b)
        with np.errstate(invalid="ignore"):
            ok = (np.isnan(g64) & np.isnan(w64)) | (g64 == w64) | (np.abs(g64 - w64) <= tol)
        assert ok.all(), f"{what}: values {gd[~ok]} != {wd[~ok]} (tol {tol[~ok]})"
    else:
        assert np.array_equal(gd, wd, equal_nan=wd.dtype.kind == "f"), f"{what}: {gd} != {wd}"


def assert_counts(want_n, got_n, what=""):
    if want_n is None:
        assert got_n is None, what
        return
    assert type(got_n) is type(want_n), f"{what}: count type {type(got_n)} != {type(want_n)}"
    assert got_n.dtype == want_n.dtype and got_n.shape == want_n.shape, what
    assert np.array_equal(got_n, want_n), f"{what}: counts {got_n} != {want_n}"


def oracle_partials(arr, sel, axis, missing):
    """Per-output (count, sum, min, max) of one chunk straight from the
    oracle (``oracle.storage_ref.reduce_chunk_bytes``: ``chunk[sel]``, then
    mask_missing, storage.py:95-100), C order over the kept dims.  Sums in
    the class accumulator (f64 / i64 / u64); min/max in the native dtype,
    NaN where an unmasked NaN is present.  Floats also get ``exact`` (the
    exactly rounded sum) and ``abs_sum`` (sum|x|) of the unmasked values.
    For checking a kernel's raw per-output partials against the reference
    semantics directly."""
    from oracle import storage_ref as ref
    dt = arr.dtype
    nd = dt.newbyteorder("=")
    if missing is None:
        missing = (None, None, None, None)
    vals, _ = ref.reduce_chunk_bytes(arr.tobytes(), None, None, missing, dt.str, arr.shape, "C", sel, axis, None)
    m = np.ma.getmaskarray(vals)
    vm = np.ma.MaskedArray(np.ma.getdata(vals).astype(nd), mask=m)
    acc = np.float64 if dt.kind == "f" else (np.int64 if dt.kind == "i" else np.uint64)
    out = {"count": (~m).sum(axis=axis, keepdims=True).reshape(-1)}
    out["sum"] = np.ma.filled(vm.astype(acc), 0).sum(axis=axis, keepdims=True).reshape(-1)
    with np.errstate(invalid="ignore"):
        out["min"] = np.ma.getdata(np.ma.min(vm, axis=axis, keepdims=True)).reshape(-1)
        out["max"] = np.ma.getdata(np.ma.max(vm, axis=axis, keepdims=True)).reshape(-1)
    if dt.kind == "f":
        ex = exact_reference(vm, axis)
        out["exact"], out["abs_sum"] = ex["exact"], ex["abs_sum"]
    return out


def assert_sums_match_exact(got_sum, vals, axis, dt, what, ok=None, old_rtol=CAP_PARTIAL[0],
                            old_atol=CAP_PARTIAL[1]):
    """Raw f64 partial sums of a float kernel against the exact sums of the
    masked selection ``vals``: within sum_bound(dt) and within the earlier
    ``old_atol + old_rtol |sum|`` rule.  Returns the worst error/bound."""
    ex = exact_reference(vals, axis)
    if ok is None:
        ok = ex["n"] > 0
    b = sum_bound(dt, ex["n"], ex["abs_sum"], "sum")[ok]
    w = ex["exact"][ok]
    with np.errstate(invalid="ignore"):
        old = old_atol + old_rtol * np.abs(w)
    return assert_within(np.asarray(got_sum, dtype=np.float64)[ok], w, b, f"{what}: sum", old=old)


def assert_reduction_close(got, vals, axis, dt, kind, what, ok=None, old_rtol=None, old_atol=0.0,
                           factor=1.0, extended=False):
    """A sum or mean (``got``: one value per output, C order over the kept
    dims) of data of dtype ``dt`` against the exact reduction of the masked
    selection ``vals``.  float64 and integer data: sum_bound (times
    ``factor``).  float32 data at result level (chunk sums rounded to f32,
    combined in f32, as the reference does): REL_TOL / ABS_FRAC.  With
    ``old_rtol`` never more than ``old_atol + old_rtol |want|``.  Outputs
    outside ``ok`` (default: n > 0) are not compared.  Returns the worst
    error/bound."""
    dt = np.dtype(dt)
    ex = exact_reference(vals, axis, extended=extended)
    n, s = ex["n"], ex["abs_sum"]
    with np.errstate(all="ignore"):
        want = ex["exact"] if kind == "sum" else ex["exact"] / np.maximum(n, 1)
        if dt.kind == "f" and dt.itemsize == 4:
            scale = s if kind == "sum" else s / np.maximum(n, 1)
            b = np.maximum(REL_TOL * np.abs(want), ABS_FRAC * scale)
            b = np.where(np.isfinite(s), b, 0.0)
        else:
            b = factor * sum_bound(np.float64, n, s, kind, mean_abs=want, extended=extended)
        old = None if old_rtol is None else old_atol + old_rtol * np.abs(want)
    if ok is None:
        ok = n > 0
    ok = np.asarray(ok).reshape(-1)
    g = np.asarray(np.ma.getdata(got), dtype=np.float64).reshape(-1)
    return assert_within(g[ok], want[ok], b[ok], what, old=None if old is None else old[ok])


def assert_partials_match_oracle(parts, want, dt, what):
    """Kernel partials (engine.partial_dtype rows) vs oracle_partials: count
    exact, min/max equal where count > 0 (NaN where NumPy gives NaN; the
    sign of a zero extreme is fixed later by the zero-sign passes, so values
    compare equal here), sums exact (integers) or within sum_bound of the
    exact sum (floats; a non-finite sum must match)."""
    nd = dt.newbyteorder("=")
    np.testing.assert_array_equal(parts["count"], want["count"], err_msg=f"{what}: count")
    ok = want["count"] > 0
    for k in ("min", "max"):
        g = parts[k][ok].astype(nd)
        w = want[k][ok]
        if dt.kind == "f":
            np.testing.assert_array_equal(np.isnan(g), np.isnan(w), err_msg=f"{what}: {k} NaN")
            fin = ~np.isnan(w)
            np.testing.assert_array_equal(g[fin], w[fin], err_msg=f"{what}: {k}")
        else:
            np.testing.assert_array_equal(g, w, err_msg=f"{what}: {k}")
    if dt.kind == "f":
        g, w = parts["sum"][ok].astype(np.float64), want["exact"][ok]
        b = sum_bound(dt, want["count"][ok], want["abs_sum"][ok], "sum")
        with np.errstate(invalid="ignore"):
            old = CAP_PARTIAL[1] + CAP_PARTIAL[0] * np.abs(w)
        return assert_within(g, w, b, f"{what}: sum", old=old)
    np.testing.assert_array_equal(parts["sum"][ok], want["sum"][ok], err_msg=f"{what}: sum")
    return 0.0
