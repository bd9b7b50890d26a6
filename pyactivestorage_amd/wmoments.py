"""Weighted second-moment records on the host: what ``Active.var`` / ``std``
/ ``cov`` / ``corr`` return with ``weights=``, and how a caller merges partial
results.

A record is ``engine.wcomoments_dtype`` (``pyas_wcomoments`` in
``include/pyas.h``): ``count`` pairs unmasked on both sides, ``sw = sum w`` and
``sw2 = sum w^2`` over them, the weighted means ``mean_x`` and ``mean_y``,
``m2_x = sum w (x - mean_x)^2``, ``m2_y`` likewise and
``cxy = sum w (x - mean_x)(y - mean_y)``, all float64.  A query over one
variable leaves ``mean_y``, ``m2_y`` and ``cxy`` 0.  The all-zero record is
neutral.
"""
from __future__ import annotations

import numpy as np

from .engine import wcomoments_dtype

_NAMES = ("count", "sw", "sw2", "mean_x", "mean_y", "m2_x", "m2_y", "cxy")


def records(count, sw, sw2, mean_x, mean_y, m2_x, m2_y, cxy) -> np.ndarray:
    """Structured records from broadcastable fields."""
    parts = np.broadcast_arrays(*(np.asarray(v) for v in (count, sw, sw2, mean_x, mean_y, m2_x, m2_y, cxy)))
    out = np.zeros(parts[0].shape, dtype=wcomoments_dtype)
    for name, v in zip(_NAMES, parts):
        out[name] = v
    return out


def of(x, w, y=None) -> np.ndarray:
    """The record of every element of ``x`` (pair of ``x`` and ``y``, same
    shape) unmasked (on both sides) under the weights ``w``, which broadcast
    against ``x`` (two passes on the host; for tests and for callers that mix
    in host data).  A NaN or an infinity at weight 0 gives NaN, as on the
    device."""
    x = np.ma.asarray(x)
    ok = ~np.ma.getmaskarray(x)
    if y is not None:
        y = np.ma.asarray(y)
        if x.shape != y.shape:
            raise ValueError(f"x and y must have the same shape. Got {x.shape} and {y.shape}")
        ok = ok & ~np.ma.getmaskarray(y)
    wv = np.broadcast_to(np.asarray(w, dtype=np.float64), x.shape)[ok]
    a = np.ma.getdata(x)[ok].astype(np.float64)
    b = np.ma.getdata(y)[ok].astype(np.float64) if y is not None else None
    if a.size == 0:
        return records(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    with np.errstate(all="ignore"):
        sw, sw2 = wv.sum(), (wv * wv).sum()
        has = sw > 0

        def side(v):
            mean = (wv * v).sum() / sw if has else 0.0
            d = v - mean
            return (mean if has else 0.0), d, (wv * d * d).sum()
        ma, da, m2a = side(a)
        if b is None:
            return records(a.size, sw, sw2, ma, 0.0, m2a, 0.0, 0.0)
        mb, db, m2b = side(b)
        return records(a.size, sw, sw2, ma, mb, m2a, m2b, (wv * da * db).sum())


def merge(a, b) -> np.ndarray:
    """The weighted Chan merge of two record arrays (broadcast against each
    other), ``a`` first.  ``count``, ``sw`` and ``sw2`` add.  Where both sides
    have ``sw > 0``, with ``d_x``, ``d_y`` the differences of the means and
    ``f = sw_b / (sw_a + sw_b)``: ``mean = mean_a + d f``,
    ``m2 = m2_a + m2_b + d d sw_a f`` and ``cxy = cxy_a + cxy_b + d_x d_y sw_a f``.
    A side with ``sw == 0`` gives no mean, but its m2s and cxy (each exactly 0,
    or NaN from a NaN at weight 0) are still added.  The m2s are clamped at 0,
    ``cxy`` is not; the empty record is neutral."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=wcomoments_dtype), np.asarray(b, dtype=wcomoments_dtype))
    both = (a["sw"] > 0) & (b["sw"] > 0)
    sw = a["sw"] + b["sw"]
    with np.errstate(all="ignore"):
        f = np.where(both, b["sw"] / np.where(both, sw, 1.0), 0.0)
        out = {}
        d = {}
        for s in ("x", "y"):
            ma, mb = a["mean_" + s], b["mean_" + s]
            d[s] = np.where(both, mb - ma, 0.0)
            out["mean_" + s] = np.where(both, ma + d[s] * f, np.where(b["sw"] > 0, mb, ma))
            m2 = a["m2_" + s] + b["m2_" + s] + d[s] * d[s] * a["sw"] * f
            out["m2_" + s] = np.where(m2 < 0, 0.0, m2)      # NaN stays NaN
        cxy = a["cxy"] + b["cxy"] + d["x"] * d["y"] * a["sw"] * f
    return records(a["count"] + b["count"], sw, a["sw2"] + b["sw2"], out["mean_x"], out["mean_y"], out["m2_x"],
                   out["m2_y"], cxy)


def _fact(parts, ddof):
    """``(sw sw - ddof sw2) / sw`` (the normaliser of ``np.cov(aweights=w,
    ddof=ddof)``) and where it gives no result: ``sw == 0`` or a numerator
    ``<= 0``."""
    sw, sw2 = parts["sw"], parts["sw2"]
    with np.errstate(all="ignore"):
        num = sw * sw - int(ddof) * sw2
        bad = (sw == 0) | ~(num > 0)
        return num / np.where(sw == 0, 1.0, sw), bad


def finalize_var(parts, ddof: int = 0, std: bool = False) -> np.ma.MaskedArray:
    """``var = m2_x / fact`` with ``fact = (sw sw - ddof sw2) / sw`` (``std``:
    its square root) as a float64 masked array of ``parts``' shape, masked
    where ``sw == 0`` or ``sw sw - ddof sw2 <= 0``; a NaN ``m2_x`` stays NaN."""
    parts = np.asarray(parts, dtype=wcomoments_dtype)
    fact, bad = _fact(parts, ddof)
    with np.errstate(all="ignore"):
        val = parts["m2_x"] / np.where(bad, 1.0, fact)
        if std:
            val = np.sqrt(val)
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)


def finalize_cov(parts, ddof: int = 0) -> np.ma.MaskedArray:
    """``cov = cxy / fact`` (see :func:`finalize_var`), masked alike; a NaN
    ``cxy`` stays NaN."""
    parts = np.asarray(parts, dtype=wcomoments_dtype)
    fact, bad = _fact(parts, ddof)
    with np.errstate(all="ignore"):
        val = parts["cxy"] / np.where(bad, 1.0, fact)
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)


def finalize_corr(parts) -> np.ma.MaskedArray:
    """The weighted centred correlation ``cxy / sqrt(m2_x) / sqrt(m2_y)``
    clipped to [-1, 1] as a float64 masked array of ``parts``' shape, masked
    where ``sw == 0``; NaN, not masked, where either m2 is 0 (0/0) or any of
    the three is NaN."""
    parts = np.asarray(parts, dtype=wcomoments_dtype)
    bad = parts["sw"] == 0
    with np.errstate(all="ignore"):
        val = parts["cxy"] / np.sqrt(parts["m2_x"]) / np.sqrt(parts["m2_y"])
        val = np.clip(val, -1.0, 1.0)      # NaN stays NaN
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)
