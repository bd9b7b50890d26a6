"""Weighted-sum records on the host: what ``Active.mean`` / ``Active.sum``
return with ``weights=``, and how a caller merges partial results.

A record is ``engine.wsum_dtype`` (``pyas_wsum`` in ``include/pyas.h``):
``count`` unmasked elements, ``sw = sum w`` and ``swx = sum w x`` over them,
float64.  The all-zero record is neutral; records merge by addition.
"""
from __future__ import annotations

import numpy as np

from .engine import wsum_dtype


def records(count, sw, swx) -> np.ndarray:
    """Structured records from broadcastable ``count``, ``sw`` and ``swx``."""
    count, sw, swx = np.broadcast_arrays(np.asarray(count), np.asarray(sw), np.asarray(swx))
    out = np.zeros(count.shape, dtype=wsum_dtype)
    out["count"] = count
    out["sw"] = sw
    out["swx"] = swx
    return out


def merge(a, b) -> np.ndarray:
    """The record of the union of two disjoint sets (arrays broadcast against
    each other), ``a`` first: each field is added."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=wsum_dtype), np.asarray(b, dtype=wsum_dtype))
    with np.errstate(all="ignore"):
        return records(a["count"] + b["count"], a["sw"] + b["sw"], a["swx"] + b["swx"])


def finalize(parts, mean: bool = True) -> np.ma.MaskedArray:
    """``mean``: ``swx / sw``, masked where ``sw == 0`` (no unmasked element,
    or every unmasked element has weight exactly 0); else the weighted sum
    ``swx``, masked where ``count == 0``.  A float64 masked array of ``parts``'
    shape; a NaN ``swx`` stays NaN."""
    parts = np.asarray(parts, dtype=wsum_dtype)
    if mean:
        bad = parts["sw"] == 0
        with np.errstate(all="ignore"):
            val = parts["swx"] / np.where(bad, 1.0, parts["sw"])
    else:
        bad = parts["count"] == 0
        val = parts["swx"]
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)
