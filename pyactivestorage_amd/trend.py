"""Least-squares trend records on the host: what ``Active.trend`` returns, and
how a caller merges partial results.

A record is ``engine.comoments_dtype`` (``pyas_comoments`` in
``include/pyas.h``) with ``x`` the coordinate along one dimension and ``y`` the
data: ``count`` unmasked elements, ``mean_x`` and ``mean_y`` over them,
``m2_x = sum (x - mean_x)^2``, ``m2_y`` likewise and
``cxy = sum (x - mean_x)(y - mean_y)``, all float64.  The least-squares line
through the counted points is ``y = intercept + slope x`` with
``slope = cxy / m2_x`` and ``intercept = mean_y - slope mean_x``.
"""
from __future__ import annotations

import numpy as np

from . import comoments
from .engine import comoments_dtype

merge = comoments.merge


def check_coord(coord, n: int) -> np.ndarray:
    """``coord`` as a float64 vector of ``n`` finite entries (``None``:
    ``arange(n)``).  ValueError when it is not numeric, not 1-D, of another
    length, or holds a NaN or an infinity.  Entries may repeat and need not be
    monotonic."""
    if coord is None:
        return np.arange(int(n), dtype=np.float64)
    try:
        c = np.asarray(coord, dtype=np.float64)
    except (TypeError, ValueError) as exc:
        raise ValueError(f"coord is not numeric: {exc}") from None
    if c.ndim != 1 or c.size != int(n):
        raise ValueError(f"coord must be 1-D with {int(n)} entries. Got shape {c.shape}")
    if not np.all(np.isfinite(c)):
        raise ValueError("coord has a NaN or infinite entry")
    return np.ascontiguousarray(c)


def of(coord_along, y, along: int) -> np.ndarray:
    """The record of every unmasked element of ``y`` (a masked array) against
    ``coord_along`` (``y.shape[along]`` entries) broadcast along dimension
    ``along`` (two passes on the host; for tests and for callers that mix in
    host data)."""
    y = np.ma.asarray(y)
    if y.ndim == 0:
        raise ValueError("y must have at least one dimension")
    if isinstance(along, (bool, np.bool_)) or not -y.ndim <= along < y.ndim:
        raise ValueError(f"along={along!r} is out of range for {y.ndim} dimensions")
    along = int(along) % y.ndim
    c = check_coord(coord_along, y.shape[along])
    shape = [1] * y.ndim
    shape[along] = c.size
    x = np.broadcast_to(c.reshape(shape), y.shape)
    return comoments.of(np.ma.MaskedArray(x, mask=np.ma.getmaskarray(y)), y)


def _parts(parts) -> np.ndarray:
    if isinstance(parts, dict):   # the components of a query
        n = np.ma.getdata(parts["n"])
        return comoments.records(n, *(np.ma.getdata(parts[k]) for k in ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")))
    return np.asarray(parts, dtype=comoments_dtype)


def slope(parts) -> np.ma.MaskedArray:
    """``cxy / m2_x`` as a float64 masked array of ``parts``' shape (records,
    or the ``components`` dict of a query): masked where ``count == 0``; NaN,
    not masked, where ``m2_x == 0`` (one counted element, or all counted
    coordinates equal) or where ``cxy`` is NaN."""
    parts = _parts(parts)
    bad = parts["count"] == 0
    with np.errstate(all="ignore"):
        val = parts["cxy"] / parts["m2_x"]
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)


def intercept(parts) -> np.ma.MaskedArray:
    """``mean_y - slope mean_x``, masked and NaN as :func:`slope`."""
    parts = _parts(parts)
    bad = parts["count"] == 0
    with np.errstate(all="ignore"):
        val = parts["mean_y"] - (parts["cxy"] / parts["m2_x"]) * parts["mean_x"]
    val = np.where(bad, 0.0, val)
    return np.ma.MaskedArray(np.ascontiguousarray(val, dtype=np.float64), mask=bad)
