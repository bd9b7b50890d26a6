"""Exceed records on the host: what ``Active.exceed`` returns, the check of a
per-output threshold field, and how a caller joins partial results (years,
files).

A record is ``engine.exceed_dtype`` (``pyas_exceed`` in ``include/pyas.h``):
``n`` unmasked and ``n_true`` true positions (int64), ``sum`` the float64 sum
of the true elements and ``excess`` the float64 sum of ``|x - threshold|`` over
them.  The all-zero record is neutral and :func:`merge` adds field by field,
so it is associative and commutative (the float fields to rounding).
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import spell
from .engine import exceed_dtype

FIELDS = ("n", "n_true", "sum", "excess")
STATS = ("count", "fraction", "sum", "mean", "excess")


def check_stat(stat) -> str:
    if not isinstance(stat, str) or stat not in STATS:
        raise ValueError(f"stat must be one of {', '.join(STATS)}. Got {stat!r}")
    return stat


def check_field(threshold, shape, axes) -> SimpleNamespace:
    """The threshold of a query over a variable of ``shape`` reduced over
    ``axes`` (sorted, non-negative).  A real scalar must be finite
    (``spell.check_threshold``).  Anything else is a per-output field:
    array-like with ``len(shape)`` dims, extent ``shape[d]`` on every kept dim
    and 1 on every reduced dim, converted to float64; its entries must be
    finite, except the masked entries of a masked array.  Returns a namespace
    of ``scalar`` (a float, or None for a field), ``values`` (the float64
    field in C order with NaN at masked entries, or None), ``mask`` (bool, the
    field's shape; None when nothing is masked) and ``all_masked`` (a
    one-entry field whose entry is masked).  A field with every dim reduced
    has one entry and is the scalar case.  ValueError otherwise."""
    shape = tuple(int(n) for n in shape)
    if np.ndim(threshold) == 0 and not isinstance(threshold, np.ma.MaskedArray):
        return SimpleNamespace(scalar=spell.check_threshold(threshold), values=None, mask=None, all_masked=False)
    mask = np.ma.getmaskarray(threshold) if isinstance(threshold, np.ma.MaskedArray) else None
    try:
        values = np.array(np.ma.getdata(threshold), dtype=np.float64, order="C")
    except (TypeError, ValueError) as exc:
        raise ValueError(f"threshold is not numeric: {exc}") from None
    want = tuple(1 if d in axes else n for d, n in enumerate(shape))
    if values.ndim != len(shape):
        raise ValueError(f"a threshold field must have {len(shape)} dimensions (shape {want}). Got shape "
                         f"{values.shape}")
    if values.shape != want:
        raise ValueError(f"a threshold field must have shape {want}: the variable's extent on every kept dimension "
                         f"and 1 on every reduced one. Got shape {values.shape}")
    if mask is not None and not mask.any():
        mask = None
    ok = np.isfinite(values) if mask is None else (np.isfinite(values) | mask)
    if not ok.all():
        raise ValueError("a threshold field must be finite everywhere (mask the entries that have no threshold)")
    if mask is not None:
        mask = np.ascontiguousarray(mask)
        values[mask] = np.nan          # nothing compares true against a NaN
    if values.size == 1 and len(axes) == len(shape):
        if mask is not None:
            return SimpleNamespace(scalar=0.0, values=None, mask=mask, all_masked=True)
        return SimpleNamespace(scalar=float(values.reshape(-1)[0]), values=None, mask=None, all_masked=False)
    return SimpleNamespace(scalar=None, values=values, mask=mask, all_masked=False)


def records(n, n_true, sum_, excess) -> np.ndarray:
    """Records from their fields (broadcast against each other)."""
    cols = np.broadcast_arrays(*(np.asarray(x) for x in (n, n_true, sum_, excess)))
    out = np.zeros(cols[0].shape, dtype=exceed_dtype)
    for name, x in zip(FIELDS, cols):
        out[name] = x
    return out


def _parts(parts) -> np.ndarray:
    if isinstance(parts, dict):   # the components of a query
        return records(*(np.ma.getdata(parts[k]) for k in FIELDS))
    return np.asarray(parts, dtype=exceed_dtype)


def merge(a, b) -> np.ndarray:
    """The records of the union of two disjoint selections (records, or the
    ``components`` dicts of two queries; broadcast against each other): every
    field adds.  Both sides must come from the same ``op`` and the same
    threshold per output; nothing here can check that."""
    a, b = np.broadcast_arrays(_parts(a), _parts(b))
    return records(a["n"] + b["n"], a["n_true"] + b["n_true"], a["sum"] + b["sum"], a["excess"] + b["excess"])


def finalize(parts, stat: str = "count", thr_masked=None) -> np.ma.MaskedArray:
    """``stat`` of ``parts`` (records, or the ``components`` dict of a query)
    as a masked array of their shape: ``count`` (``n_true``, int64),
    ``fraction`` (``n_true / n``), ``sum``, ``excess`` (float64), masked where
    ``n == 0``; ``mean`` (``sum / n_true``, float64) masked where
    ``n_true == 0``.  ``thr_masked``: a bool array (broadcast against the
    records) of the outputs whose threshold is masked; the result is masked
    there too.  A masked value is 0."""
    stat = check_stat(stat)
    p = _parts(parts)
    n, nt = p["n"], p["n_true"]
    bad = (nt == 0) if stat == "mean" else (n == 0)
    if thr_masked is not None:
        bad = bad | np.broadcast_to(np.asarray(thr_masked, dtype=bool), p.shape)
    if stat == "count":
        return np.ma.MaskedArray(np.ascontiguousarray(np.where(bad, 0, nt), dtype=np.int64), mask=bad)
    with np.errstate(divide="ignore", invalid="ignore"):
        if stat == "fraction":
            val = nt.astype(np.float64) / n.astype(np.float64)
        elif stat == "sum":
            val = p["sum"]
        elif stat == "mean":
            val = p["sum"] / nt.astype(np.float64)
        else:
            val = p["excess"]
    return np.ma.MaskedArray(np.ascontiguousarray(np.where(bad, 0.0, val), dtype=np.float64), mask=bad)
