"""Exact order statistics on the host: the keys ``Active.quantile`` selects
on, the ranks and the interpolation of ``np.quantile``, and the NumPy
statement of the device's radix select.

Key rule (``include/pyas.h``): every element maps to an unsigned key whose
order is the order of the values.  1-, 2- and 4-byte types use a 32-bit key,
8-byte types a 64-bit one.  Unsigned integers are their own key (widened);
signed integers are widened to the key's width and have their sign bit
flipped; floats add 0 first (``-0.0`` becomes ``+0.0``), then flip every bit
if the sign bit is set and set the sign bit otherwise.  NaN has no key: it is
counted apart before keying.

Select: the key of the ``rank``-th smallest element (zero-based) is found
most significant digit first.  A pass counts, for every element, the digit at
``shift`` of the keys that agree with the prefix found so far above that digit;
keys with a smaller part above count as *below*, with a larger as *above*.
The digit whose running count (starting at *below*) first exceeds the rank
extends the prefix.  After the last digit the prefix is the key.
"""
from __future__ import annotations

import numpy as np

# Digit width of a pass, 1..MAX_BITS: a table row has 2^bits + 3 slots.  A
# query narrows it until its table fits histogram.TABLE_CAP_BYTES.
DIGIT_BITS = 8
MAX_BITS = 11            # 2^11 slots: the most the LDS form of the count kernel holds

METHODS = ("linear", "lower", "higher", "midpoint", "nearest")


def key_width(dtype) -> int:
    """32 or 64: the bits of the key of ``dtype``."""
    dt = np.dtype(dtype)
    if dt.kind not in "iuf" or dt.itemsize not in (1, 2, 4, 8) or (dt.kind == "f" and dt.itemsize < 4):
        raise TypeError(f"no key for dtype {dt}")
    return 64 if dt.itemsize == 8 else 32


def keys(x) -> np.ndarray:
    """The order-preserving unsigned keys (uint32 or uint64) of ``x`` (no NaN)."""
    x = np.asarray(x)
    w = key_width(x.dtype)
    x = x.astype(x.dtype.newbyteorder("="), copy=False)
    ut = np.uint64 if w == 64 else np.uint32
    sign = ut(1) << ut(w - 1)
    if x.dtype.kind == "u":
        return x.astype(ut)
    if x.dtype.kind == "i":
        return x.astype(np.int64 if w == 64 else np.int32).view(ut) ^ sign
    u = (x + x.dtype.type(0)).view(ut)
    return np.where(u & sign != 0, ~u, u | sign)


def values(k, dtype) -> np.ndarray:
    """The inverse of :func:`keys`: the values of ``dtype`` (native byte order) with keys ``k``."""
    dt = np.dtype(dtype).newbyteorder("=")
    w = key_width(dt)
    ut = np.uint64 if w == 64 else np.uint32
    k = np.asarray(k).astype(ut)
    sign = ut(1) << ut(w - 1)
    if dt.kind == "u":
        return k.astype(dt)
    if dt.kind == "i":
        return (k ^ sign).view(np.int64 if w == 64 else np.int32).astype(dt)
    return np.where(k & sign != 0, k ^ sign, ~k).view(dt)


def digits(width: int, bits: int):
    """The ``(shift, bits)`` of every pass over a ``width``-bit key, most
    significant first; the last digit may be narrower (32 = 11 + 11 + 10)."""
    if not 1 <= bits <= MAX_BITS:
        raise ValueError(f"digit width {bits} outside 1..{MAX_BITS}")
    out, left = [], width
    while left > 0:
        b = min(bits, left)
        left -= b
        out.append((left, b))
    return out


def fit_bits(n_rows: int, cap_bytes: int, want: int | None = None) -> int:
    """The largest digit width <= ``want`` (default DIGIT_BITS) whose table of
    ``n_rows`` rows x (2^bits + 3) int64 fits ``cap_bytes``; ValueError when
    even 1-bit digits do not."""
    want = DIGIT_BITS if want is None else int(want)
    if not 1 <= want <= MAX_BITS:
        raise ValueError(f"DIGIT_BITS = {want} outside 1..{MAX_BITS}")
    for b in range(want, 0, -1):
        if n_rows * ((1 << b) + 3) * 8 <= cap_bytes:
            return b
    raise ValueError(f"quantile table of {n_rows} outputs x (2 + 3) slots takes {n_rows * 5 * 8} bytes, "
                     f"above the cap of {cap_bytes} bytes")


def check_q(q) -> np.ndarray:
    """``q`` as float64 (0-D or 1-D, every entry in [0, 1]); ValueError otherwise."""
    try:
        qs = np.asarray(q, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"q must be a number or a 1-D sequence of numbers in [0, 1]. Got {q!r}") from None
    if qs.ndim > 1:
        raise ValueError(f"q must be a scalar or 1-D. Got shape {qs.shape}")
    if not np.all((qs >= 0) & (qs <= 1)):     # NaN fails both
        raise ValueError(f"q must lie in [0, 1]. Got {q!r}")
    return qs


def check_method(method) -> str:
    if method not in METHODS:
        raise ValueError(f"Bad quantile 'method': {method!r}. Choose from {'/'.join(METHODS)}.")
    return method


def ranks(n, q, method="linear"):
    """``(h, r_lo, r_hi)`` for ``n`` values and quantiles ``q`` (they broadcast):
    NumPy's virtual index ``h = (n - 1) * q`` (float64, one multiply) and the
    zero-based ranks of the two order statistics ``method`` reads: ``floor(h)``
    and ``ceil(h)`` for ``linear`` and ``midpoint``, and twice the same rank
    for ``lower`` (floor), ``higher`` (ceil) and ``nearest`` (``np.around``:
    half to even).  Ranks are clipped to ``[0, max(n - 1, 0)]``."""
    check_method(method)
    n = np.asarray(n, dtype=np.int64)
    h = (n - 1) * np.asarray(q, dtype=np.float64)
    top = np.broadcast_to(np.maximum(n - 1, 0), h.shape)
    lo, hi = np.floor(h), np.ceil(h)
    if method == "lower":
        hi = lo
    elif method == "higher":
        lo = hi
    elif method == "nearest":
        lo = hi = np.around(h)
    r_lo = np.clip(lo.astype(np.int64), 0, top)
    r_hi = np.clip(hi.astype(np.int64), 0, top)
    return h, r_lo, r_hi


def finalize(v_lo, v_hi, h, method="linear"):
    """NumPy's ``_lerp`` of the two order statistics (float64) at virtual
    index ``h``: ``g = h - floor(h)`` (``midpoint``: 0.5 where ``g > 0``),
    ``d = b - a``, ``b - d (1 - g)`` where ``g >= 0.5`` and ``a + d g``
    elsewhere.  ``lower``, ``higher`` and ``nearest`` return ``v_lo``."""
    check_method(method)
    a = np.asarray(v_lo, dtype=np.float64)
    if method in ("lower", "higher", "nearest"):
        return a.copy()
    b = np.asarray(v_hi, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    g = h - np.floor(h)
    if method == "midpoint":
        g = np.where(g > 0, 0.5, 0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return np.where(g >= 0.5, b - d * (1 - g), a + d * g)


def select(k, rank: int, bits: int):
    """The device algorithm in NumPy: ``(key, tables)`` of the ``rank``-th
    smallest (zero-based) of the keys ``k`` (uint32 or uint64, 1-D, not
    empty), with digits of ``bits`` bits.  ``tables``: one int64 row per pass,
    ``2^b`` digit counts then below, above, nan (0 here), ``b`` the pass's
    digit width."""
    k = np.asarray(k).reshape(-1)
    if k.dtype not in (np.dtype(np.uint32), np.dtype(np.uint64)):
        raise TypeError(f"keys must be uint32 or uint64. Got {k.dtype}")
    if not 0 <= rank < k.size:
        raise ValueError(f"rank {rank} outside 0..{k.size - 1}")
    width = k.dtype.itemsize * 8
    k64 = k.astype(np.uint64)
    prefix, tables = 0, []
    for shift, b in digits(width, bits):
        top = shift + b
        hi = np.zeros_like(k64) if top >= 64 else k64 >> np.uint64(top)
        on = hi == np.uint64(prefix)
        row = np.zeros((1 << b) + 3, dtype=np.int64)
        dig = ((k64[on] >> np.uint64(shift)) & np.uint64((1 << b) - 1)).astype(np.int64)
        row[:1 << b] = np.bincount(dig, minlength=1 << b)
        row[1 << b] = int((hi < np.uint64(prefix)).sum())
        row[(1 << b) + 1] = int((hi > np.uint64(prefix)).sum())
        tables.append(row)
        run = row[1 << b] + np.cumsum(row[:1 << b])
        j = int(np.searchsorted(run, rank, side="right"))     # the first digit whose running count exceeds rank
        prefix = (prefix << b) | j
    return k.dtype.type(prefix), tables
