"""Arg-extreme records on the host: what ``Active.argmax`` / ``Active.argmin``
return, and how a caller joins partial results (years, files) that lie along the
reduced dimension.

A record is ``engine.argext_dtype`` (``pyas_argext`` in ``include/pyas.h``):
``value``, the bits of the winning element in the data's class (floats as
float64, signed integers as int64, unsigned as uint64: :func:`values` reads
them), ``index``, its index along the dimension, and ``n``, the count of
unmasked elements.  An element beats another when it is a NaN and the other is
not, or when neither is a NaN and it is larger (``max``) / smaller (``min``) in
the data's class; among equals (two NaNs, ``-0.0`` and ``+0.0``) the smaller
index wins.  A record with ``n == 0`` is neutral.  :func:`merge` is associative
and commutative.
"""
from __future__ import annotations

import numpy as np

from .engine import argext_dtype

FIELDS = ("value", "index", "n")
WHICH = ("max", "min")
_CLASS = {"f": np.dtype("<f8"), "i": np.dtype("<i8"), "u": np.dtype("<u8")}


def check_which(which) -> str:
    if not isinstance(which, str) or which not in WHICH:
        raise ValueError(f"which must be one of {', '.join(WHICH)}. Got {which!r}")
    return which


def check_dtype(dtype) -> np.dtype:
    """The data's dtype; ValueError when it is not a real numeric type."""
    dt = np.dtype(dtype)
    if dt.kind not in _CLASS:
        raise ValueError(f"dtype must be an integer or a float type. Got {dt}")
    return dt


def check_along(along, ndim: int) -> int:
    """``along`` as a non-negative dimension of ``ndim``."""
    if isinstance(along, (bool, np.bool_)) or not isinstance(along, (int, np.integer)) or not -ndim <= along < ndim:
        raise ValueError(f"along={along!r} is out of range for {ndim} dimensions")
    return int(along) % ndim


def records(value, index, n, dtype) -> np.ndarray:
    """Records from their fields (broadcast against each other); ``value`` in
    the data's ``dtype`` (any byte order), carried in its class."""
    cls = _CLASS[check_dtype(dtype).kind]
    cols = np.broadcast_arrays(np.asarray(value), np.asarray(index), np.asarray(n))
    out = np.zeros(cols[0].shape, dtype=argext_dtype)
    out["value"] = cols[0].astype(cls, order="C").view("<u8")
    out["index"] = cols[1]
    out["n"] = cols[2]
    empty = out["n"] == 0                       # the neutral record is all zero
    out["value"][empty] = 0
    out["index"][empty] = 0
    return out


def values(parts, dtype) -> np.ndarray:
    """The ``value`` field of records as an array of the data's (native)
    ``dtype``, bit for bit the winning elements."""
    dt = check_dtype(dtype).newbyteorder("=")
    p = np.asarray(parts, dtype=argext_dtype)
    return p["value"].copy().view(_CLASS[dt.kind]).astype(dt)


def _parts(parts, dtype) -> np.ndarray:
    if isinstance(parts, dict):   # the components of a query
        return records(np.ma.getdata(parts["value"]), np.ma.getdata(parts["index"]), np.ma.getdata(parts["n"]), dtype)
    return np.asarray(parts, dtype=argext_dtype)


def of(data, valid_mask, along: int, which: str) -> np.ndarray:
    """The records of an array on the host, one per sequence along dimension
    ``along`` (which is dropped): ``valid_mask`` marks the unmasked elements
    (``None``: all); ``index`` is the position along ``along``.  For tests and
    for callers that mix in host data."""
    x = np.asarray(data)
    if x.ndim == 0:
        raise ValueError("data must have at least one dimension")
    dt = check_dtype(x.dtype)
    which = check_which(which)
    v = np.ones(x.shape, dtype=bool) if valid_mask is None else np.asarray(valid_mask, dtype=bool)
    if v.shape != x.shape:
        raise ValueError(f"valid_mask has shape {v.shape}, data {x.shape}")
    d = check_along(along, x.ndim)
    x = np.moveaxis(x, d, 0).astype(dt.newbyteorder("="))
    v = np.moveaxis(v, d, 0)
    if x.shape[0] >= 2 ** 31:
        raise NotImplementedError("sequences of 2^31 positions or more")
    shape = x.shape[1:]
    best = np.zeros(shape, dtype=x.dtype)
    idx = np.zeros(shape, dtype=np.int64)
    n = np.zeros(shape, dtype=np.int64)
    for i, (row, ok) in enumerate(zip(x, v)):      # the device lane's walk, vectorised over the sequences
        with np.errstate(invalid="ignore"):
            better = (row > best) if which == "max" else (row < best)
            if dt.kind == "f":
                better |= np.isnan(row) & ~np.isnan(best)
        take = ok & ((n == 0) | better)
        best = np.where(take, row, best)
        idx = np.where(take, i, idx)
        n += ok
    return records(best, idx, n, dt)


def merge(a, b, shift: int = 0, *, which: str, dtype=None) -> np.ndarray:
    """The records of the sets of ``a`` and ``b`` together (records, or the
    ``components`` dicts of two queries; broadcast against each other);
    ``shift`` is added to ``b``'s indices (the length of what lies before
    ``b`` along the dimension).  ``which``: ``"max"`` or ``"min"``, as the
    records were made; ``dtype``: the data's, which the values are compared in
    (taken from ``value`` when ``a`` is a components dict)."""
    if dtype is None:
        if not isinstance(a, dict):
            raise ValueError("dtype is needed to compare the values of plain records")
        dtype = np.ma.getdata(a["value"]).dtype
    dt = check_dtype(dtype)
    which = check_which(which)
    a, b = np.broadcast_arrays(_parts(a, dt), _parts(b, dt))
    cls = _CLASS[dt.kind]
    va, vb = (r["value"].copy().view(cls) for r in (a, b))
    ia, ib = a["index"].astype(np.int64), b["index"].astype(np.int64) + int(shift)
    na, nb = a["n"].astype(np.int64), b["n"].astype(np.int64)
    # (one index is one element; the bits only make the order total for records of any origin)
    first = (ib < ia) | ((ib == ia) & (b["value"] < a["value"]))
    with np.errstate(invalid="ignore"):
        better = (vb > va) if which == "max" else (vb < va)
        beats = better | ((vb == va) & first)
        if dt.kind == "f":
            an, bn = np.isnan(va), np.isnan(vb)
            beats = np.where(an | bn, bn & (~an | first), beats)
    take_b = (na == 0) | ((nb != 0) & beats)
    if ((na + nb >= 2 ** 31) | (np.where(take_b, ib, ia) >= 2 ** 31)).any():
        raise NotImplementedError("sequences of 2^31 positions or more")
    out = np.zeros(a.shape, dtype=argext_dtype)
    out["value"] = np.where(take_b, b["value"], a["value"])
    out["index"] = np.where(take_b, ib, ia)
    out["n"] = na + nb
    empty = out["n"] == 0
    out["value"][empty] = 0
    out["index"][empty] = 0
    return out


def finalize(parts) -> np.ma.MaskedArray:
    """The index of ``parts`` (records, or the ``components`` dict of a query)
    as an int64 masked array of their shape, masked where ``n == 0``."""
    if isinstance(parts, dict):
        index, n = np.ma.getdata(parts["index"]), np.ma.getdata(parts["n"])
    else:
        p = np.asarray(parts, dtype=argext_dtype)
        index, n = p["index"], p["n"]
    bad = np.asarray(n) == 0
    return np.ma.MaskedArray(np.where(bad, 0, index).astype(np.int64), mask=bad)
