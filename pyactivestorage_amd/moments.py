"""Second-moment records on the host: what ``Active.var`` / ``Active.std``
return, and how a caller merges partial results.

A record is ``engine.moments_dtype`` (``pyas_moments`` in ``include/pyas.h``):
``count`` unmasked elements, their ``mean`` and ``m2 = sum (x - mean)^2``,
all float64.  ``count == 0`` is neutral.
"""
from __future__ import annotations

import numpy as np

from .engine import moments_dtype


def records(count, mean, m2) -> np.ndarray:
    """Structured records from broadcastable ``count``, ``mean`` and ``m2``."""
    count, mean, m2 = np.broadcast_arrays(np.asarray(count), np.asarray(mean), np.asarray(m2))
    out = np.zeros(count.shape, dtype=moments_dtype)
    out["count"] = count
    out["mean"] = mean
    out["m2"] = m2
    return out


def of(values) -> np.ndarray:
    """The record of every unmasked element of ``values`` (two passes on the
    host; for tests and for callers that mix in host data)."""
    a = np.ma.compressed(np.ma.asarray(values)).astype(np.float64)
    if a.size == 0:
        return records(0, 0.0, 0.0)
    mean = a.mean()
    return records(a.size, mean, ((a - mean) ** 2).sum())


def merge(a, b) -> np.ndarray:
    """Chan's merge of two record arrays (broadcast against each other), ``a``
    first: ``d = mean_b - mean_a``, ``mean = mean_a + d n_b / n``,
    ``m2 = m2_a + m2_b + d^2 n_a n_b / n``.  A side with ``count == 0`` is
    skipped, so the empty record is neutral."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=moments_dtype), np.asarray(b, dtype=moments_dtype))
    na, nb = a["count"].astype(np.float64), b["count"].astype(np.float64)
    n = na + nb
    with np.errstate(all="ignore"):
        d = b["mean"] - a["mean"]
        w = nb / np.where(n == 0, 1.0, n)
        mean = a["mean"] + d * w
        m2 = a["m2"] + b["m2"] + d * d * na * w
    out = records(a["count"] + b["count"], mean, m2)
    skip_b, skip_a = b["count"] == 0, (a["count"] == 0) & (b["count"] != 0)
    out[skip_b] = a[skip_b]
    out[skip_a] = b[skip_a]
    out["reserved"] = 0
    return out


def finalize(parts, ddof: int = 0, std: bool = False) -> np.ma.MaskedArray:
    """``var = m2 / (count - ddof)`` (``std``: its square root) as a float64
    masked array of ``parts``' shape, masked where ``count - ddof <= 0``; a
    NaN ``m2`` stays NaN."""
    parts = np.asarray(parts, dtype=moments_dtype)
    dof = parts["count"] - int(ddof)
    bad = dof <= 0
    with np.errstate(all="ignore"):
        val = parts["m2"] / np.where(bad, 1, dof).astype(np.float64)
        if std:
            val = np.sqrt(val)
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)
