"""Spell records on the host: what ``Active.spell`` returns, and how a caller
joins partial results (years, files) that follow each other along the spell
dimension.

A record is ``engine.spell_dtype`` (``pyas_spell`` in ``include/pyas.h``), ten
int32 about the runs of *true* positions in a sequence of selected positions:
``n`` unmasked and ``n_true`` true positions, ``len`` positions covered,
``head`` / ``tail`` the length of the leading / trailing run (both ``len`` when
every position is true), ``best`` the longest run, ``days`` / ``events`` the
total length / number of the *interior* runs (those that touch neither end) of
length >= ``min_length``, and ``min_length`` itself.  The all-zero record is
neutral.  :func:`merge` is associative but not commutative: ``a`` comes before
``b``.
"""
from __future__ import annotations

import numpy as np

from .engine import spell_dtype

FIELDS = ("n", "n_true", "len", "head", "tail", "best", "days", "events", "min_length")
OPS = ("gt", "ge", "lt", "le")
STATS = ("longest", "days", "events")


def check_op(op) -> str:
    if not isinstance(op, str) or op not in OPS:
        raise ValueError(f"op must be one of {', '.join(OPS)}. Got {op!r}")
    return op


def check_threshold(threshold) -> float:
    """``threshold`` as a finite float.  ValueError when it is not a real
    number, a NaN or an infinity."""
    if isinstance(threshold, (bool, np.bool_)) or not isinstance(threshold, (int, float, np.integer, np.floating)):
        raise ValueError(f"threshold must be a finite number. Got {threshold!r}")
    t = float(threshold)
    if not np.isfinite(t):
        raise ValueError(f"threshold must be a finite number. Got {threshold!r}")
    return t


def check_min_length(min_length) -> int:
    if isinstance(min_length, (bool, np.bool_)) or not isinstance(min_length, (int, np.integer)) \
            or not 1 <= min_length < 2 ** 31:
        raise ValueError(f"min_length must be an int >= 1. Got {min_length!r}")
    return int(min_length)


def check_stat(stat) -> str:
    if not isinstance(stat, str) or stat not in STATS:
        raise ValueError(f"stat must be one of {', '.join(STATS)}. Got {stat!r}")
    return stat


def records(n, n_true, len_, head, tail, best, days, events, min_length) -> np.ndarray:
    """Records from their fields (broadcast against each other)."""
    cols = np.broadcast_arrays(*(np.asarray(x) for x in (n, n_true, len_, head, tail, best, days, events, min_length)))
    out = np.zeros(cols[0].shape, dtype=spell_dtype)
    for name, x in zip(FIELDS, cols):
        out[name] = x
    return out


def _parts(parts) -> np.ndarray:
    if isinstance(parts, dict):   # the components of a query
        return records(*(np.ma.getdata(parts[k]) for k in FIELDS))
    return np.asarray(parts, dtype=spell_dtype)


def of(true_mask, valid_mask, along: int, min_length: int = 1) -> np.ndarray:
    """The records of boolean arrays on the host, one per sequence along
    dimension ``along`` (which is dropped): ``true_mask`` marks the true
    positions, ``valid_mask`` the unmasked ones (``None``: all); a position
    that is not valid is not true.  For tests and for callers that mix in host
    data."""
    t = np.asarray(true_mask, dtype=bool)
    if t.ndim == 0:
        raise ValueError("true_mask must have at least one dimension")
    v = np.ones(t.shape, dtype=bool) if valid_mask is None else np.asarray(valid_mask, dtype=bool)
    if v.shape != t.shape:
        raise ValueError(f"valid_mask has shape {v.shape}, true_mask {t.shape}")
    if isinstance(along, (bool, np.bool_)) or not -t.ndim <= along < t.ndim:
        raise ValueError(f"along={along!r} is out of range for {t.ndim} dimensions")
    L = check_min_length(min_length)
    t = np.moveaxis(t & v, int(along) % t.ndim, 0)
    v = np.moveaxis(v, int(along) % v.ndim, 0)
    if t.shape[0] >= 2 ** 31:
        raise NotImplementedError("sequences of 2^31 positions or more")
    shape = t.shape[1:]
    cur, head, best, days, events = (np.zeros(shape, dtype=np.int64) for _ in range(5))
    broken = np.zeros(shape, dtype=bool)
    for row in t:                       # the device lane's walk, vectorised over the sequences
        close = ~row
        interior = close & broken & (cur >= L)
        head = np.where(close & ~broken, cur, head)
        days += np.where(interior, cur, 0)
        events += interior
        broken |= close
        cur = np.where(close, 0, cur + 1)
        best = np.maximum(best, cur)
    n_len = np.full(shape, t.shape[0], dtype=np.int64)
    return records(v.sum(axis=0), t.sum(axis=0), n_len, np.where(broken, head, n_len), cur, best, days, events, L)


def merge(a, b) -> np.ndarray:
    """The records of the sequences of ``a`` followed by those of ``b``
    (records, or the ``components`` dicts of two queries; broadcast against
    each other).  The order matters."""
    a, b = np.broadcast_arrays(_parts(a), _parts(b))
    f = lambda r, k: r[k].astype(np.int64)
    L = np.maximum(f(a, "min_length"), f(b, "min_length"))
    a_all, b_all = a["head"] == a["len"], b["head"] == b["len"]
    j = f(a, "tail") + f(b, "head")
    joined = ~a_all & ~b_all & (j >= L)
    out = records(f(a, "n") + f(b, "n"), f(a, "n_true") + f(b, "n_true"), f(a, "len") + f(b, "len"),
                  np.where(a_all, f(a, "len") + f(b, "head"), f(a, "head")),
                  np.where(b_all, f(b, "len") + f(a, "tail"), f(b, "tail")),
                  np.maximum(np.maximum(f(a, "best"), f(b, "best")), j),
                  f(a, "days") + f(b, "days") + np.where(joined, j, 0),
                  f(a, "events") + f(b, "events") + joined, L)
    if (f(a, "len") + f(b, "len") >= 2 ** 31).any():
        raise NotImplementedError("sequences of 2^31 positions or more")
    return out


def finalize(parts, stat: str = "longest") -> np.ma.MaskedArray:
    """``longest``, ``days`` or ``events`` of ``parts`` (records, or the
    ``components`` dict of a query) as an int64 masked array of their shape,
    masked where ``n == 0``: the leading and the trailing run count here, once
    nothing more is to be merged."""
    stat = check_stat(stat)
    p = _parts(parts)
    f = lambda k: p[k].astype(np.int64)
    L, head, tail = f("min_length"), f("head"), f("tail")
    h = (head >= L) & (head > 0)
    t = (head != f("len")) & (tail >= L) & (tail > 0)
    if stat == "longest":
        val = f("best")
    elif stat == "days":
        val = f("days") + np.where(h, head, 0) + np.where(t, tail, 0)
    else:
        val = f("events") + h + t
    bad = p["n"] == 0
    return np.ma.MaskedArray(np.ascontiguousarray(np.where(bad, 0, val), dtype=np.int64), mask=bad)
