"""Binned counts on the host: the edges ``Active.histogram`` bins with, the
NumPy statement of its bin rule, and what a caller does with the counts.

Bin rule (``include/pyas.h``): with ``n + 1`` strictly increasing finite
float64 edges ``e``, a float64 value ``x`` counts in bin ``i`` when
``e[i] <= x < e[i+1]``; the last bin also holds ``x == e[n]``; ``x < e[0]``
and ``-inf`` count as *below*, ``x > e[n]`` and ``+inf`` as *above*, NaN as
*nan*.  This is ``np.histogram(x64, bins=e)`` on the float64 copy of the data.
"""
from __future__ import annotations

import numpy as np

MAX_BINS = 1 << 20       # PYAS_HIST_MAX_BINS
# Most bytes of a query's device table, n_outputs x (n_bins + 3) x 8 (Active.histogram raises above it)
TABLE_CAP_BYTES = 2 << 30


def _check_range(range_):
    try:
        lo, hi = range_
        lo, hi = float(lo), float(hi)
    except (TypeError, ValueError):
        raise ValueError(f"range must be a (lo, hi) pair of numbers. Got {range_!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"range {range_!r} is not finite")
    if lo > hi:
        raise ValueError(f"range: lo must not exceed hi. Got {range_!r}")
    if lo == hi:             # as NumPy does
        lo, hi = lo - 0.5, hi + 0.5
    return lo, hi


def is_count(bins) -> bool:
    """Whether ``bins`` is a bin count (an int, not a bool) and not an edge sequence."""
    return isinstance(bins, (int, np.integer)) and not isinstance(bins, (bool, np.bool_))


def edges(bins, range=None) -> np.ndarray:   # noqa: A002 - NumPy's argument name
    """The float64 bin edges of ``bins``: for an int ``n >= 1`` with
    ``range = (lo, hi)`` they are ``np.linspace(lo, hi, n + 1)`` (``lo == hi``
    becomes ``(lo - 0.5, hi + 0.5)``); a sequence gives its own edges (1-D, at
    least 2, finite, strictly increasing; ``range`` is then not used).
    ValueError for anything else, for a non-finite range, ``lo > hi`` and for
    more than ``MAX_BINS`` bins."""
    if is_count(bins):
        n = int(bins)
        if n < 1:
            raise ValueError(f"bins must be an int >= 1 or a sequence of edges. Got {bins!r}")
        if n > MAX_BINS:
            raise ValueError(f"bins = {n} exceeds the most bins of a histogram, {MAX_BINS}")
        if range is None:
            raise ValueError("range is required with an int number of bins")
        lo, hi = _check_range(range)
        e = np.linspace(lo, hi, n + 1)
        if not np.all(np.diff(e) > 0):
            raise ValueError(f"range {range!r} is too narrow for {n} distinct float64 bin edges")
        return e
    if isinstance(bins, (bool, np.bool_, str, bytes)) or bins is None:
        raise ValueError(f"bins must be an int >= 1 or a sequence of edges. Got {bins!r}")
    try:
        e = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"bins must be an int >= 1 or a sequence of edges. Got {bins!r}") from None
    if e.ndim != 1 or e.size < 2:
        raise ValueError(f"bin edges must be 1-D with at least 2 entries. Got shape {e.shape}")
    if not np.all(np.isfinite(e)):
        raise ValueError("bin edges must be finite")
    if not np.all(np.diff(e) > 0):
        raise ValueError("bin edges must be strictly increasing (equal neighbours are not allowed)")
    if e.size - 1 > MAX_BINS:
        raise ValueError(f"{e.size - 1} bins exceed the most bins of a histogram, {MAX_BINS}")
    return e


def bin_counts(x64, bin_edges):
    """The bin rule in NumPy: ``(counts, below, above, nan)`` of the float64
    values ``x64`` (any shape; every element counts) over ``bin_edges``;
    ``counts`` is int64 with ``len(bin_edges) - 1`` entries, the rest are ints."""
    x = np.asarray(x64, dtype=np.float64).reshape(-1)
    e = np.asarray(bin_edges, dtype=np.float64)
    n = e.size - 1
    nan = int(np.isnan(x).sum())
    with np.errstate(invalid="ignore"):
        below = int((x < e[0]).sum())
        above = int((x > e[n]).sum())
        inside = x[(x >= e[0]) & (x <= e[n])]
    idx = np.searchsorted(e, inside, side="right") - 1   # the largest i with e[i] <= x
    idx[idx == n] = n - 1                                 # x == e[n]: the last bin is closed
    counts = np.bincount(idx, minlength=n).astype(np.int64)
    return counts, below, above, nan


def merge(a, b):
    """The histogram of two disjoint sets of elements from their histograms:
    addition.  ``a`` and ``b`` are count arrays of one shape, or the dicts
    ``Active.histogram`` returns with ``components`` (their ``bin_edges`` must
    be equal)."""
    if isinstance(a, dict) or isinstance(b, dict):
        if not (isinstance(a, dict) and isinstance(b, dict)):
            raise ValueError("merge: both sides must be count arrays or both component dicts")
        if not np.array_equal(a["bin_edges"], b["bin_edges"]):
            raise ValueError("merge: the two histograms have different bin edges")
        out = {k: merge(a[k], b[k]) for k in ("counts", "n", "below", "above", "nan")}
        out["bin_edges"] = np.array(a["bin_edges"], dtype=np.float64)
        return out
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        raise ValueError(f"merge: shapes {a.shape} and {b.shape} differ")
    return a.astype(np.int64) + b.astype(np.int64)


def quantile(counts, bin_edges, q):
    """Approximate quantiles of the binned values (those inside the edges).
    With ``N`` values counted, rank ``k = q N`` falls in the bin ``i`` whose
    cumulative counts satisfy ``cum[i] < k <= cum[i+1]``; the result is
    ``e[i] + (k - cum[i]) / counts[i] * (e[i+1] - e[i])``, linear inside that
    bin.  The ``ceil(k)``-th smallest value lies in the same bin, so the result
    is within one bin width of it.  ``counts``: ``(..., n_bins)``; ``q``: a
    scalar or 1-D in [0, 1].  Returns float64 of shape ``counts.shape[:-1] +
    q.shape``; NaN where nothing was counted.  For the exact order
    statistics of a variable use ``Active.quantile`` / ``Active.median`` (a
    radix select on the device, equal to ``np.quantile``)."""
    c = np.asarray(counts, dtype=np.int64)
    e = np.asarray(bin_edges, dtype=np.float64)
    qs = np.asarray(q, dtype=np.float64)
    if c.ndim < 1 or e.ndim != 1 or c.shape[-1] != e.size - 1:
        raise ValueError(f"counts {c.shape} do not fit {e.size} bin edges")
    if qs.ndim > 1 or np.any(~((qs >= 0) & (qs <= 1))):
        raise ValueError("q must be a scalar or 1-D with values in [0, 1]")
    rows = c.reshape(-1, c.shape[-1])
    qf = qs.reshape(-1)
    out = np.full((rows.shape[0], qf.size), np.nan)
    for r, row in enumerate(rows):
        cum = np.concatenate([[0], np.cumsum(row)])
        total = cum[-1]
        if total == 0:
            continue
        k = qf * float(total)
        i = np.searchsorted(cum[1:], k, side="left")          # first bin with cum[i+1] >= k
        i = np.minimum(i, row.size - 1)
        first = int(np.flatnonzero(row)[0])
        i = np.where(k <= 0, first, i)                         # q = 0: the first occupied bin's left edge
        frac = (k - cum[i]) / np.maximum(row[i], 1)
        out[r] = e[i] + np.clip(frac, 0.0, 1.0) * (e[i + 1] - e[i])
    return out.reshape(c.shape[:-1] + qs.shape)
