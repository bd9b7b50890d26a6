"""Per-label statistics on the host: what ``Active.grouped`` checks, the
tables its two kernels walk, and how its records become a result.

A record is ``engine.moments_dtype`` (``pyas_moments`` in ``include/pyas.h``),
one per (output, group): the ``count``, ``mean`` and ``m2`` of the selected
unmasked elements whose label is the group's number.  ``labels`` has one
integer per global index along the labelled dimension; a negative label puts
the index in no group.  ``moments.merge`` combines the records of disjoint
selections.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from . import moments
from .dtypes import native, sum_dtype
from .engine import moments_dtype

STATS = ("mean", "var", "std", "count", "min", "max", "sum")
# the stats whose record is ``engine.partial_dtype`` (``pyas_partial``): per
# (output, group) the sum, the count and the NaN-propagating min and max
PARTIAL_STATS = ("min", "max", "sum")

merge = moments.merge


def _pmin(a, b):
    """NaN-propagating minimum, elementwise, in the arrays' own type."""
    if a.dtype.kind == "f":
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b < a, b, a)))
    return np.where(b < a, b, a)


def _pmax(a, b):
    if a.dtype.kind == "f":
        return np.where(np.isnan(a), a, np.where(np.isnan(b), b, np.where(b > a, b, a)))
    return np.where(b > a, b, a)


def merge_partials(a, b):
    """The ``engine.partial_dtype`` records of the union of two disjoint
    selections, elementwise (broadcast): sums and counts added (integer sums
    wrap modulo 2^64 as NumPy's do), min and max NaN-propagating in the
    records' own type; a side with ``count == 0`` is skipped, whatever its
    other fields hold.  What ``moments.merge`` is to the other stats."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.dtype.names != ("sum", "count", "min", "max"):
        raise ValueError(f"merge_partials: two arrays of one engine.partial_dtype. Got {a.dtype} and {b.dtype}")
    a, b = np.broadcast_arrays(a, b)
    out = np.zeros(a.shape, dtype=a.dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        out["sum"] = a["sum"] + b["sum"]
    out["count"] = a["count"] + b["count"]
    out["min"] = _pmin(a["min"], b["min"])
    out["max"] = _pmax(a["max"], b["max"])
    ea, eb = a["count"] == 0, b["count"] == 0
    out[eb] = a[eb]
    only_b = ea & ~eb
    out[only_b] = b[only_b]
    return out


def check_labels(labels, n: int, n_groups=None):
    """``labels`` as an int64 vector of ``n`` entries and the group count
    ``G``: ``n_groups``, or ``max(labels) + 1`` (0 when every label is
    negative) for None.  ValueError when the labels are not a 1-D integer
    array-like of ``n`` entries (floats and bools are refused), when
    ``n_groups`` is not a non-negative int, or when a label is ``>= n_groups``."""
    a = np.asarray(labels)
    if a.dtype.kind not in "iu":
        raise ValueError(f"labels must be integers. Got dtype {a.dtype}")
    if a.ndim != 1 or a.size != int(n):
        raise ValueError(f"labels must be 1-D with {int(n)} entries. Got shape {a.shape}")
    if a.dtype.kind == "u" and a.size and int(a.max()) >= 2 ** 31:
        raise ValueError("labels of 2^31 or more")
    a = np.ascontiguousarray(a, dtype=np.int64)
    top = int(a.max()) if a.size else -1
    if top >= 2 ** 31:
        raise ValueError("labels of 2^31 or more")
    if n_groups is None:
        return a, max(top + 1, 0)
    if isinstance(n_groups, (bool, np.bool_)) or not isinstance(n_groups, (int, np.integer)) or n_groups < 0:
        raise ValueError(f"n_groups must be a non-negative int. Got {n_groups!r}")
    if top >= n_groups:
        raise ValueError(f"a label is {top} with n_groups={int(n_groups)}")
    if n_groups >= 2 ** 31:
        raise ValueError("n_groups of 2^31 or more")
    return a, int(n_groups)


def _local(p) -> np.ndarray:
    """The indices inside the chunk that projection ``p`` selects, in the
    order of its positions."""
    s = p.chunk_sel
    if isinstance(s, slice):
        return np.arange(s.start, s.stop, s.step, dtype=np.int64)[:len(p.out_pos)]
    return np.asarray(s, dtype=np.int64).reshape(-1)


def row_list(red_dims, chunks, labels, along: int, n_groups: int):
    """The sorted row list of the dense path (pyas_group_rows).  ``red_dims``:
    the projections of the reduced dims ``0 .. P-1`` of a box query (per dim,
    one projection per chunk coordinate the selection touches); ``chunks``: the
    chunk shape; ``labels``: the checked labels along dim ``along < P``.

    A row is one position of the reduced dims' selection.  Returns a namespace
    of ``layer`` (the C-order position of the row's chunk over the reduced
    dims' chunk coordinates), ``offset`` (its element offset inside the chunk:
    the reduced dims' indices inside the chunk times the chunk's row-major
    element strides), ``label`` (the label of its global index along
    ``along``), all int32 over the rows whose label is ``>= 0``, sorted stably
    by label and inside a label by global position (C order over the reduced
    dims' global indices); ``starts`` (int64, ``n_groups + 1``: group ``g`` is
    rows ``starts[g]:starts[g+1]``) and ``n_rows``.  All columns of chunks
    share the list: a box selects the same reduced rows in each."""
    P = len(red_dims)
    chunks = [int(c) for c in chunks]
    cstride = [int(np.prod(chunks[d + 1:])) for d in range(len(chunks))]
    per_dim = []
    for d, projs in enumerate(red_dims):
        coord, local, glob = [], [], []
        for a, p in enumerate(projs):
            li = _local(p)
            coord.append(np.full(li.size, a, dtype=np.int64))
            local.append(li)
            glob.append(li + int(p.chunk_ix) * chunks[d])
        cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
        per_dim.append((cat(coord), cat(local), cat(glob), len(projs)))
    n_rows_all = int(np.prod([x[0].size for x in per_dim])) if per_dim else 0
    layer = np.zeros(n_rows_all, dtype=np.int64)
    offset = np.zeros(n_rows_all, dtype=np.int64)
    order_key = np.zeros(n_rows_all, dtype=np.int64)
    label = np.zeros(n_rows_all, dtype=np.int64)
    if n_rows_all:
        grids = np.meshgrid(*[np.arange(x[0].size) for x in per_dim], indexing="ij")
        for d, (coord, local, glob, n_coord) in enumerate(per_dim):
            k = grids[d].reshape(-1)
            layer = layer * n_coord + coord[k]
            offset += local[k] * cstride[d]
            order_key = order_key * (int(glob.max()) + 1) + glob[k]
            if d == along:
                label = labels[glob[k]]
    keep = np.nonzero(label >= 0)[0]
    keep = keep[np.lexsort((order_key[keep], label[keep]))]
    if keep.size and (int(offset.max()) >= 2 ** 31 or int(layer.max()) >= 2 ** 31):
        raise NotImplementedError("chunks of 2^31 elements or more")
    out = SimpleNamespace(layer=layer[keep].astype(np.int32), offset=offset[keep].astype(np.int32),
                          label=label[keep].astype(np.int32), n_rows=int(keep.size))
    out.starts = np.searchsorted(out.label, np.arange(int(n_groups) + 1)).astype(np.int64)
    return out


def chunk_lists(chunk_projs, chunks, labels, along: int, axes, final_shape, n_groups: int):
    """The per-chunk group lists of the walk path (pyas_group_lists) and the
    segments that send its records to their final places.  ``chunk_projs``:
    per chunk, in launch order, its per-dim projections; ``final_shape``: the
    query's result shape with 1 along every reduced dim.

    Chunk ``c`` has the local groups ``chunk_start[c]:chunk_start[c+1]``, one
    per label ``>= 0`` present among its selected indices along ``along``, in
    increasing label order (``group_label``: their labels); local group ``j``
    holds ``pos[ptr[j]:ptr[j+1]]``, the positions among the chunk's *selected*
    indices along ``along`` that carry its label, increasing.  The kernel
    writes chunk ``c``'s records at ``out_off[c] + j * n_keep + o`` (``j`` from
    0 inside the chunk, ``o`` in C order over its ``n_keep`` kept selected
    positions); record ``order[seg[f]:seg[f+1]]`` combine, in chunk order, to
    entry ``f`` of the result, whose shape is ``final_shape`` with
    ``n_groups`` along ``along``.  Returns a namespace of ``chunk_start``,
    ``ptr``, ``pos`` (int32), ``group_label`` (int64), ``out_off`` (int64,
    one entry per chunk and the total), ``order`` and ``seg`` (int64)."""
    chunks = [int(c) for c in chunks]
    rshape = tuple(int(n_groups) if d == along else int(n) for d, n in enumerate(final_shape))
    chunk_start, ptr, pos, glabel, sizes, fidx = [0], [0], [], [], [], []
    for projs in chunk_projs:
        p = projs[along]
        lab = labels[_local(p) + int(p.chunk_ix) * chunks[along]]
        present = np.unique(lab[lab >= 0])
        for g in present:
            where = np.nonzero(lab == g)[0]
            pos.append(where)
            ptr.append(ptr[-1] + where.size)
        glabel.append(present)
        chunk_start.append(chunk_start[-1] + present.size)
        kept = [np.asarray(pr.out_pos, dtype=np.int64) if d not in axes else np.zeros(1, dtype=np.int64)
                for d, pr in enumerate(projs)]
        kept[along] = present.astype(np.int64)
        # the records' order: the local group slowest, then C order over the kept dims
        grids = np.meshgrid(*([kept[along]] + [k for d, k in enumerate(kept) if d != along]), indexing="ij")
        multi = [None] * len(kept)
        multi[along] = grids[0].reshape(-1)
        rest = iter(grids[1:])
        for d in range(len(kept)):
            if d != along:
                multi[d] = next(rest).reshape(-1)
        fidx.append(np.ravel_multi_index(multi, rshape) if multi[0].size else np.zeros(0, dtype=np.int64))
        sizes.append(multi[0].size)
    cat = lambda parts: np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)
    f_all = cat(fidx).astype(np.int64, copy=False)
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    if ptr[-1] >= 2 ** 31 or chunk_start[-1] >= 2 ** 31:
        raise NotImplementedError("group lists of 2^31 entries or more")
    order = np.argsort(f_all, kind="stable").astype(np.int64)
    seg = np.searchsorted(f_all[order], np.arange(int(np.prod(rshape)) + 1)).astype(np.int64)
    return SimpleNamespace(chunk_start=np.asarray(chunk_start, dtype=np.int32), ptr=np.asarray(ptr, dtype=np.int32),
                           pos=cat(pos).astype(np.int32), group_label=cat(glabel).astype(np.int64),
                           out_off=out_off, order=order, seg=seg)


def finalize(parts, stat: str, ddof: int = 0, dtype=None):
    """The result of a grouped query from its records: ``count`` the int64
    counts (never masked); ``mean`` a float64 masked array, masked where
    ``count == 0`` and NaN where a counted value is NaN or infinite; ``var`` /
    ``std`` ``moments.finalize``: masked where ``count - ddof <= 0``.
    ``min`` / ``max`` / ``sum`` take ``engine.partial_dtype`` records and the
    variable's ``dtype`` (None: the records' own 8-byte class): ``min`` and
    ``max`` in the variable's dtype in native byte order, ``sum`` in
    ``dtypes.sum_dtype`` (an f32 variable's f64 sum rounded once), each a
    masked array with a full mask, masked (and 0) where ``count == 0``."""
    if stat not in STATS:
        raise ValueError(f"stat must be one of {STATS}. Got {stat!r}")
    if stat in PARTIAL_STATS:
        parts = np.asarray(parts)
        if parts.dtype.names != ("sum", "count", "min", "max"):
            raise ValueError(f"stat {stat!r} takes engine.partial_dtype records. Got {parts.dtype}")
        vdt = parts.dtype[stat] if dtype is None else (sum_dtype(dtype) if stat == "sum" else native(dtype))
        empty = parts["count"] == 0
        with np.errstate(over="ignore"):   # (an f64 sum beyond f32 rounds to an infinity, as NumPy's f32 sum ends)
            val = np.ascontiguousarray(parts[stat]).astype(vdt)
        val[empty] = 0
        return np.ma.MaskedArray(val, mask=empty)
    parts = np.asarray(parts, dtype=moments_dtype)
    if stat == "count":
        return np.ascontiguousarray(parts["count"], dtype=np.int64)
    if stat == "mean":
        empty = parts["count"] == 0
        # a counted NaN or infinity leaves a NaN m2 (an infinity that is not the
        # lane's first element leaves an infinite mean): NaN, as for var and std
        val = np.where(np.isnan(parts["m2"]), np.nan, parts["mean"])
        return np.ma.MaskedArray(np.where(empty, 0.0, val).astype(np.float64), mask=empty)
    return moments.finalize(parts, ddof, std=stat == "std")
