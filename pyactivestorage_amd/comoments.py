"""Co-moment records on the host: what ``Active.cov`` / ``Active.corr``
return, and how a caller merges partial results.

A record is ``engine.comoments_dtype`` (``pyas_comoments`` in
``include/pyas.h``): ``count`` pairs unmasked on both sides, their ``mean_x``
and ``mean_y``, ``m2_x = sum (x - mean_x)^2``, ``m2_y`` likewise and
``cxy = sum (x - mean_x)(y - mean_y)``, all float64.  ``count == 0`` is
neutral.
"""
from __future__ import annotations

import numpy as np

from .engine import comoments_dtype

_FIELDS = ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")


def records(count, mean_x, mean_y, m2_x, m2_y, cxy) -> np.ndarray:
    """Structured records from broadcastable fields."""
    parts = np.broadcast_arrays(*(np.asarray(v) for v in (count, mean_x, mean_y, m2_x, m2_y, cxy)))
    out = np.zeros(parts[0].shape, dtype=comoments_dtype)
    for name, v in zip(("count",) + _FIELDS, parts):
        out[name] = v
    return out


def of(x, y) -> np.ndarray:
    """The record of every pair of ``x`` and ``y`` (same shape) unmasked on
    both sides (two passes on the host; for tests and for callers that mix in
    host data)."""
    x, y = np.ma.asarray(x), np.ma.asarray(y)
    if x.shape != y.shape:
        raise ValueError(f"x and y must have the same shape. Got {x.shape} and {y.shape}")
    ok = ~(np.ma.getmaskarray(x) | np.ma.getmaskarray(y))
    a = np.ma.getdata(x)[ok].astype(np.float64)
    b = np.ma.getdata(y)[ok].astype(np.float64)
    if a.size == 0:
        return records(0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        ma, mb = a.mean(), b.mean()
        da, db = a - ma, b - mb
        return records(a.size, ma, mb, (da * da).sum(), (db * db).sum(), (da * db).sum())


def merge(a, b) -> np.ndarray:
    """Chan's merge of two record arrays (broadcast against each other), ``a``
    first: with ``d_x``, ``d_y`` the differences of the means,
    ``cxy = cxy_a + cxy_b + d_x d_y n_a n_b / n`` and the means and m2s as
    ``moments.merge``.  A side with ``count == 0`` is skipped, so the empty
    record is neutral."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=comoments_dtype), np.asarray(b, dtype=comoments_dtype))
    na, nb = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = na + nb
    with np.errstate(all="ignore"):
        dx, dy = b["mean_x"] - a["mean_x"], b["mean_y"] - a["mean_y"]
        w = nb / np.where(n == 0, 1.0, n)
        out = records(a["count"] + b["count"], a["mean_x"] + dx * w, a["mean_y"] + dy * w,
                      a["m2_x"] + b["m2_x"] + dx * dx * na * w, a["m2_y"] + b["m2_y"] + dy * dy * na * w,
                      a["cxy"] + b["cxy"] + dx * dy * na * w)
    skip_b, skip_a = b["count"] == 0, (a["count"] == 0) & (b["count"] != 0)
    out[skip_b] = a[skip_b]
    out[skip_a] = b[skip_a]
    return out


def finalize_cov(parts, ddof: int = 0) -> np.ma.MaskedArray:
    """``cov = cxy / (count - ddof)`` as a float64 masked array of ``parts``'
    shape, masked where ``count - ddof <= 0``; a NaN ``cxy`` stays NaN."""
    parts = np.asarray(parts, dtype=comoments_dtype)
    dof = parts["count"] - int(ddof)
    bad = dof <= 0
    with np.errstate(all="ignore"):
        val = parts["cxy"] / np.where(bad, 1, dof).astype(np.float64)
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)


def finalize_corr(parts) -> np.ma.MaskedArray:
    """Pearson's ``r = cxy / sqrt(m2_x) / sqrt(m2_y)`` clipped to [-1, 1] (as
    ``np.corrcoef`` clips) as a float64 masked array of ``parts``' shape,
    masked where ``count == 0``; NaN, not masked, where either m2 is 0 (0/0)
    or any of the three is NaN."""
    parts = np.asarray(parts, dtype=comoments_dtype)
    bad = parts["count"] == 0
    with np.errstate(all="ignore"):
        val = parts["cxy"] / np.sqrt(parts["m2_x"]) / np.sqrt(parts["m2_y"])
        val = np.clip(val, -1.0, 1.0)      # NaN stays NaN
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)
