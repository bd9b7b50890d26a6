"""Running-window records on the host: what ``Active.rolling`` returns, and how
a caller joins partial results (years, files) that follow each other along the
window dimension, so that Rx5day sees the windows across New Year.

A *window* is ``w`` positions consecutive in the selection; it is *valid* when
all ``w`` elements are unmasked (a NaN is data, not a masked element).  A valid
window's sum is ``s = f64(x[p]); s += f64(x[p+1]); ...; s += f64(x[p+w-1])``:
``w - 1`` float64 additions, oldest element first.  This order is the
definition; nothing is added and subtracted along the way.

A record is ``engine.roll_dtype`` (``pyas_roll`` in ``include/pyas.h``, 144
bytes) about one piece of a sequence: ``best`` the extreme valid-window sum and
``position`` that window's first element within the piece (both 0 when
``n_windows == 0``), ``n_windows`` valid windows, ``n`` unmasked positions,
``len`` positions, ``window`` and ``which`` (0 max, 1 min) themselves,
``head[j]`` the piece's element ``j`` and ``tail[k]`` its element
``len - 1 - k`` (the *last* element is ``tail[0]``) for
``j, k < min(len, w - 1)``, and one bit per slot in ``head_ok`` / ``tail_ok``:
the element exists and is unmasked.  Slots that do not exist or are masked hold
0, so equal pieces give equal bytes.  The all-zero record is neutral.
:func:`merge` is associative but not commutative: ``a`` comes before ``b``.
Among equal sums the first window wins (``-0.0 == +0.0``); the first NaN sum
wins over everything, as in ``np.max`` / ``np.min``.
"""
from __future__ import annotations

import numpy as np

from .engine import roll_dtype

MAX_WINDOW = 8   # include/pyas.h PYAS_ROLL_MAX_WINDOW
FIELDS = ("best", "position", "n_windows", "n", "len", "window", "which", "head_ok", "tail_ok", "head", "tail")
STATS = ("sum", "mean")
EXTREMES = ("max", "min")
_H = MAX_WINDOW - 1


def check_window(window) -> int:
    """``window`` as an int in ``1 .. MAX_WINDOW``.  ValueError when it is not
    an int >= 1, NotImplementedError when it is past the cap."""
    if isinstance(window, (bool, np.bool_)) or not isinstance(window, (int, np.integer)) or window < 1:
        raise ValueError(f"window must be an int >= 1. Got {window!r}")
    if window > MAX_WINDOW:
        raise NotImplementedError(f"window={int(window)}: windows of more than {MAX_WINDOW} positions "
                                  f"(the record keeps {MAX_WINDOW - 1} elements at either end)")
    return int(window)


def check_stat(stat) -> str:
    if not isinstance(stat, str) or stat not in STATS:
        raise ValueError(f"stat must be one of {', '.join(STATS)}. Got {stat!r}")
    return stat


def check_extreme(extreme) -> str:
    if not isinstance(extreme, str) or extreme not in EXTREMES:
        raise ValueError(f"extreme must be one of {', '.join(EXTREMES)}. Got {extreme!r}")
    return extreme


def _parts(parts) -> np.ndarray:
    if isinstance(parts, dict):   # the components of a query
        shape = np.shape(np.ma.getdata(parts["best"]))
        out = np.zeros(shape, dtype=roll_dtype)
        for name in FIELDS:
            out[name] = np.ma.getdata(parts[name])
        return out
    return np.asarray(parts, dtype=roll_dtype)


def _beats(c, best, has, mn):
    """Does the later candidate replace the holder?  Strictly better only;
    the first NaN wins and stays."""
    with np.errstate(invalid="ignore"):
        better = (c < best) if mn else (c > best)
    return ~has | (~np.isnan(best) & (np.isnan(c) | better))


def of(values, valid_mask, along: int, window: int, which: str = "max") -> np.ndarray:
    """The records of host arrays, one per sequence along dimension ``along``
    (which is dropped): ``values`` in any real dtype (each element converts as
    ``astype(float64)`` does), ``valid_mask`` the unmasked positions (``None``:
    all).  For tests and for callers that mix in host data."""
    x = np.asarray(values)
    if x.ndim == 0:
        raise ValueError("values must have at least one dimension")
    v = np.ones(x.shape, dtype=bool) if valid_mask is None else np.asarray(valid_mask, dtype=bool)
    if v.shape != x.shape:
        raise ValueError(f"valid_mask has shape {v.shape}, values {x.shape}")
    if isinstance(along, (bool, np.bool_)) or not -x.ndim <= along < x.ndim:
        raise ValueError(f"along={along!r} is out of range for {x.ndim} dimensions")
    w, mn = check_window(window), check_extreme(which) == "min"
    x = np.moveaxis(x, int(along) % x.ndim, 0).astype(np.float64)
    v = np.moveaxis(v, int(along) % v.ndim, 0)
    n_pos = x.shape[0]
    if n_pos >= 2 ** 31:
        raise NotImplementedError("sequences of 2^31 positions or more")
    out = np.zeros(x.shape[1:], dtype=roll_dtype)
    best = np.zeros(out.shape, dtype=np.float64)
    pos = np.zeros(out.shape, dtype=np.int64)
    nw = np.zeros(out.shape, dtype=np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(n_pos - w + 1):
            valid = v[p:p + w].all(axis=0)
            s = x[p].copy()
            for j in range(1, w):
                s = s + x[p + j]
            take = valid & _beats(s, best, nw > 0, mn)
            best = np.where(take, s, best)
            pos = np.where(take, p, pos)
            nw += valid
    out["best"], out["position"], out["n_windows"] = best, pos, nw
    out["n"], out["len"], out["window"], out["which"] = v.sum(axis=0), n_pos, w, int(mn)
    for j in range(min(n_pos, w - 1)):
        out["head"][..., j] = np.where(v[j], x[j], 0.0)
        out["head_ok"] |= v[j].astype(np.uint8) << j
        out["tail"][..., j] = np.where(v[n_pos - 1 - j], x[n_pos - 1 - j], 0.0)
        out["tail_ok"] |= v[n_pos - 1 - j].astype(np.uint8) << j
    return out


def _grown(first, first_n, second, h):
    """Slot ``j`` of ``first`` (``first_n`` slots) followed by ``second``, cut
    at ``h`` slots (arrays of trailing extent 7; absent slots hold 0)."""
    j = np.arange(_H)
    k = j - first_n[..., None]
    tail = np.take_along_axis(second, np.clip(k, 0, _H - 1), axis=-1)
    return np.where(k < 0, first, np.where((k < _H) & (j < h[..., None]), tail, 0.0))


def merge(a, b) -> np.ndarray:
    """The records of the sequences of ``a`` followed by those of ``b``
    (records, or the ``components`` dicts of two queries; broadcast against
    each other).  The order matters.  Every window across the seam is summed
    by the rule of this module from ``a``'s tail and ``b``'s head."""
    a, b = np.broadcast_arrays(_parts(a), _parts(b))
    i64 = lambda r, k: r[k].astype(np.int64)
    w = np.maximum(i64(a, "window"), i64(b, "window"))
    h = np.maximum(w - 1, 0)
    mn_each = (a["which"] | b["which"]) != 0
    a_len, b_len = i64(a, "len"), i64(b, "len")
    if (a_len + b_len >= 2 ** 31).any():
        raise NotImplementedError("sequences of 2^31 positions or more")
    ta, hb = np.minimum(a_len, h), np.minimum(b_len, h)
    a_tok, b_hok = i64(a, "tail_ok"), i64(b, "head_ok")
    best, pos, nw = a["best"].astype(np.float64), i64(a, "position"), i64(a, "n_windows")

    def beats(c, best, has):
        return np.where(mn_each, _beats(c, best, has, True), _beats(c, best, has, False))
    with np.errstate(invalid="ignore", over="ignore"):
        for m in range(_H, 0, -1):          # m elements of a's end, w - m of b's start: sequence order
            tneed, hneed = (1 << m) - 1, (1 << np.clip(w - m, 0, _H)) - 1
            valid = (m <= h) & ((a_tok & tneed) == tneed) & ((b_hok & hneed) == hneed)
            s = a["tail"][..., m - 1].astype(np.float64)
            for j in range(m - 2, -1, -1):
                s = s + a["tail"][..., j]
            for j in range(_H):
                s = np.where(j < w - m, s + b["head"][..., j], s)
            take = valid & beats(s, best, nw > 0)
            best = np.where(take, s, best)
            pos = np.where(take, a_len - m, pos)
            nw = nw + valid
    take = (b["n_windows"] > 0) & beats(b["best"], best, nw > 0)
    best = np.where(take, b["best"], best)
    pos = np.where(take, a_len + i64(b, "position"), pos)
    nw = nw + i64(b, "n_windows")
    out = np.zeros(a.shape, dtype=roll_dtype)
    out["best"], out["position"], out["n_windows"] = best, pos, nw
    out["n"], out["len"], out["window"], out["which"] = i64(a, "n") + i64(b, "n"), a_len + b_len, w, mn_each
    out["head"] = _grown(a["head"], ta, b["head"], h)
    out["tail"] = _grown(b["tail"], hb, a["tail"], h)
    hmask = (1 << h) - 1
    out["head_ok"] = (i64(a, "head_ok") | (b_hok << ta)) & hmask
    out["tail_ok"] = (i64(b, "tail_ok") | (a_tok << hb)) & hmask
    return out


def finalize(parts, stat: str = "sum") -> np.ma.MaskedArray:
    """The extreme window ``sum`` of ``parts`` (records, or the ``components``
    dict of a query), or the extreme window ``mean`` (that sum divided once by
    ``float64(window)``: division by a positive constant is monotone), as a
    float64 masked array of their shape, masked where there is no valid
    window."""
    stat = check_stat(stat)
    p = _parts(parts)
    bad = p["n_windows"] == 0
    val = p["best"].astype(np.float64)
    if stat == "mean":
        with np.errstate(invalid="ignore", divide="ignore"):
            val = val / np.maximum(p["window"], 1).astype(np.float64)
    return np.ma.MaskedArray(np.ascontiguousarray(np.where(bad, 0.0, val), dtype=np.float64), mask=bad)
