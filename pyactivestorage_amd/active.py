"""Batched ``Active`` front end: one device launch chain per query.

Mirrors ``activestorage/active.py``'s user API (``Active(path, ncvar)``,
``Active.method``, ``.mean()/.min()/.max()/.sum(axis)``, ``.components``,
``active[index]``, ``active.py:162-427``).  The dataset is a netCDF4/HDF5
path, whose metadata and chunk index :mod:`.hdf5` reads (pyfive's part in
the reference), or a :class:`~pyactivestorage_amd.variable.ChunkedVariable`.
``__getitem__`` replaces ``_get_selection`` + ``_from_storage``
(``active.py:439-635``):

1. plan: orthogonal indexer -> per-dim projections; for box queries the
   selection table, index pool and chunk list follow by broadcasting;
2. ingest: for a file on disk, native pread threads (``max_threads``, like
   ``active.py:557``) into pinned slots copied H2D as they fill
   (``pyas_read_ranges``, row f2); zlib chunks are inflated on the device
   (``pyas_inflate``, row f3) in stream groups that overlap the reads;
   ``resident=True`` keeps decoded chunks in HBM across queries;
3. device: one fused reduce over every chunk (full-axis queries) or a
   partial-axis reduce plus the grid combine (``pyas_combine_grid``; host
   segments via ``pyas_combine_segments`` otherwise), with per-chunk sums
   rounded to the variable dtype first, like the reference's ``out`` array
   (``active.py:512,585``);
4. ``group=``: each rank of a torch.distributed group does 2-3 for its
   contiguous share of the chunks, then one all-gather and a rank-order
   device combine (row e);
5. host: format the combined partials exactly like ``active.py:591-630``.

Beyond the reference: ``.var(axis, ddof)`` / ``.std(axis, ddof)``, one pass of
count / mean / m2 records (``pyas_moments_axes``) merged with Chan's formula
in the order the sums are combined in (``_reduce_moments``);
``.mean(axis, weights={dim: vector})`` / ``.sum(axis, weights=...)``, count /
sum w / sum w x records (``pyas_wsum_axes``) merged by addition
(``_reduce_weighted``); ``.histogram(bins, range, axis)``, int64 counts
added by every chunk straight into the result table (``pyas_hist_axes``,
``_reduce_hist``); and ``.quantile(q, axis, method)`` / ``.median(axis)``,
exact order statistics by a radix select over keys, a few passes of digit
counts in the histogram's table (``pyas_select_axes``, ``pyas_select_step``,
``_reduce_select``); and ``.cov(other, axis, ddof)`` / ``.corr(other, axis)``
over a second ``Active``, one pass of count / means / m2s / cxy records over
both variables' chunks (``pyas_comoments_axes``) merged like the var records
(``_reduce_comoments``).
"""
from __future__ import annotations

import concurrent.futures
import itertools
import os
import threading
from types import SimpleNamespace

import warnings

import numpy as np

from . import _lib, argext, comoments, engine, exceed, grouped, histogram, moments, quantile, rolling, selection, spell, \
    trend, weighted, wmoments, zerosign
from .batch import ReductionPlan, _all_full
from .device import DeviceBuffer, get_context
from .dtypes import native, sum_dtype
from .indexing import OrthogonalIndexer, _normalize
from .ingest import read_ranges, read_ranges_zlib
from .inflate import InflateBatch, is_zlib, pack_streams
from .masking import compile_missing
from .storage import _decompress, _shuffle_sizes
from .variable import ChunkedVariable, decode_filters, get_missing_attributes

_ALIGN = 256
_RECORD_SEG = 64   # records a thread folds per level of a full record reduction (var, weighted, cov, trend)
_RESIDENT_LOCK = threading.Lock()
_RESIDENT_CV = threading.Condition(_RESIDENT_LOCK)   # slot state changes
_EMPTY, _LOADING, _LOADED = 0, 1, 2


# PYAS_AXES_FOLD=0 keeps whole-chunk box queries on the two-step path
# (pyas_reduce_axes + pyas_combine_grid), for A/B measurements
_AXES_FOLD = os.environ.get("PYAS_AXES_FOLD", "1") != "0"


# Resident repeat queries: per-store cache of device plans, keyed by the
# query (index of slices/Ellipsis, reduced axes, missing-data values)
_PLAN_CACHE_CAP = 64
_MISS = object()


def _index_key(index):
    """Hashable form of an index made of slices, Ellipsis and 1-D integer
    index lists (the box queries a plan can be replayed for); None
    otherwise."""
    if not isinstance(index, tuple):
        index = (index,)
    out = []
    for x in index:
        if x is Ellipsis:
            out.append(("e",))
        elif isinstance(x, (list, np.ndarray)):
            a = np.asarray(x)
            if a.ndim != 1 or a.dtype.kind not in "iu":
                return None
            out.append(("l",) + tuple(int(v) for v in a))
        elif isinstance(x, slice):
            part = ["s"]
            for v in (x.start, x.stop, x.step):
                if v is None:
                    part.append(None)
                elif isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
                    part.append(int(v))
                else:
                    return None
            out.append(tuple(part))
        else:
            return None
    return tuple(out)


def _missing_key(missing):
    key = []
    for m in missing:
        if m is None:
            key.append(None)
        else:
            a = np.asarray(m)
            key.append((a.dtype.str, a.shape, a.tobytes()))
    return tuple(key)


class _CachedQuery:
    """A resident query's device plan, replayed by later identical queries:
    no indexer, no chunk table, no uploads or allocations, only the
    launches, the result copy and the formatting (``active.py:591-630``)."""

    def __init__(self, plan, final_shape, grid=None):
        self.plan = plan
        self.final_shape = final_shape
        self.grid = grid            # None: full reduction; else _grid_partials' record
        self.fmt = {}               # format buffers by result dtype / components
        # one replay at a time: the plan's device buffers (partials, total,
        # tie flags, result buffers) are shared by every replay of this key
        self.lock = threading.Lock()

    def run(self, act):
        with self.lock:
            return self._run(act)

    def _run(self, act):
        ctx = self.plan.ctx
        st = ctx.thread_stream()
        shape = self.final_shape
        if self.grid is None:
            final = act._total(self.plan, st)
            return act._format(final.reshape(shape), shape)
        g = self.grid
        if g["folded"]:
            g["tie"]["fused"] = act._fold(ctx, st, self.plan, g["g"], g["fin"].ptr, g["zs_ok"])
        else:   # records of this replay's method (one size per dtype: the buffer fits every method)
            g["rec"] = engine.method_rec(act._method)
            g["zs1"] = act._reduce_axes_zs(ctx, st, self.plan, g["axes_mask"], g["obuf"].ptr, g["parts"].ptr,
                                           g["rec"], g.get("zs_ok1", False))
            g["zs2"] = act._combine_zs(ctx, st, g["parts"].ptr, g["g"], g["fin"].ptr, g["rec"], g["zs1"])
        act._tie_grid(ctx, st, self.plan, g)
        return act._format_device(ctx, st, g["fin"], g["n_final"], shape, bufs=self.fmt)


def release_resident(variable) -> None:
    """Free the HBM copy that resident-mode ``Active`` queries keep for
    ``variable`` (e.g. after the file changed).  Queries already using the
    copy keep it until they finish; the last one frees it."""
    with _RESIDENT_LOCK:
        store = getattr(variable, "_pyas_resident", None)
        if store is None:
            return
        variable._pyas_resident = None
        store["released"] = True
        free = store["users"] == 0
    if free:
        store["buf"].free()


class _External:
    """A device buffer owned by the caller (attach_resident): never freed here."""

    def __init__(self, ptr, owner):
        self.ptr = int(ptr)
        self.owner = owner          # keeps the caller's allocation alive

    def free(self):
        self.owner = None


def _check_attached(variable, device) -> None:
    """A caller-attached resident copy serves queries on its own device only
    (replacing it would drop the caller's allocation behind their back)."""
    store = getattr(variable, "_pyas_resident", None)
    if store is not None and store["device"] != device and isinstance(store["buf"], _External):
        raise ValueError(f"the variable's resident copy was attached on device {store['device']}, "
                         f"not on this query's device {device} (attach_resident)")


def attach_resident(variable, ptr, device: int = 0, owner=None) -> None:
    """Register chunks already decoded in HBM as ``variable``'s resident copy:
    ``ptr`` holds every chunk of the variable's grid in C order, one slot of
    ``ceil(chunk_bytes / 256) * 256`` bytes each, in the variable's dtype
    and byte order (variables without filters only).  Resident-mode queries on
    ``variable`` then read only HBM, as if an earlier query had loaded every
    chunk (a producer on the GPU handing its output to the reduction without
    a trip through a file).  ``owner`` (e.g. the torch tensor behind ``ptr``)
    is kept alive until :func:`release_resident`."""
    ds = variable
    if ds.filter_pipeline:
        raise NotImplementedError("attach_resident: variables with a filter pipeline")
    if int(ptr) % _ALIGN:
        raise ValueError(f"attach_resident: ptr must be {_ALIGN}-byte aligned (chunk slots of the resident layout)")
    grid = tuple(-(-s // c) for s, c in zip(ds.shape, ds.chunks))
    n_all = int(np.prod(grid))
    with _RESIDENT_LOCK:
        if getattr(ds, "_pyas_resident", None) is not None:
            raise ValueError("the variable already has a resident copy (release_resident first)")
        ds._pyas_resident = {"device": int(device), "buf": _External(ptr, owner),
                             "state": np.full(n_all, _LOADED, dtype=np.int8), "users": 0,
                             "released": False}


def _unhold(store) -> None:
    """A query that used ``store`` has finished (its stream is synchronised)."""
    with _RESIDENT_LOCK:
        store["users"] -= 1
        free = store["users"] == 0 and store["released"]
    if free:
        store["buf"].free()


# read -> inflate pipeline stages of a compressed query (PYAS_INFLATE_GROUPS)
_INFLATE_GROUPS = int(os.environ.get("PYAS_INFLATE_GROUPS", "3"))

# Where Active inflates zlib chunks when device_inflate="auto" (row f3).  One
# pyas_inflate stream is one serial DEFLATE decoder (~135 MB/s, two waves per
# stream), so the device finishes up to ~2048 streams in about one stream's
# time, while the host inflates on its reader threads -- one per pinned
# staging slot in flight, min(threads, 16) -- at zlib's per-core rate and
# takes ceil(n / lanes) stream times: the device wins from about lanes x
# (host rate / device rate) streams.  Measured on MI355X with
# tools/bench_inflate_crossover.py (profiles/r06/crossover/);
# PYAS_INFLATE_CROSSOVER overrides the streams per host lane below which the
# host inflates.
_INFLATE_CROSSOVER = float(os.environ.get("PYAS_INFLATE_CROSSOVER", "10"))
_INGEST_LANES = 16   # pinned staging slots of pyas_read_ranges (ingest.py set_slots)


def inflate_on_device(n_streams: int, threads: int, mode="auto") -> bool:
    """The device/host choice for one query's zlib chunks: ``mode`` True /
    False force it; "auto" inflates on the device from ``_INFLATE_CROSSOVER``
    streams per host inflate lane (PYAS_ACTIVE_INFLATE=device|host overrides
    "auto")."""
    if mode == "auto":
        mode = {"device": True, "host": False}.get(os.environ.get("PYAS_ACTIVE_INFLATE", ""), "auto")
    if mode != "auto":
        return bool(mode)
    lanes = max(1, min(int(threads), _INGEST_LANES))
    return n_streams >= _INFLATE_CROSSOVER * lanes


def _pipeline_groups(sizes, n_groups):
    """Up to ``n_groups`` contiguous index ranges of about equal total size."""
    z = np.asarray(sizes, dtype=np.int64)
    if z.size == 0:
        return []
    cum = np.cumsum(z)
    cuts = np.searchsorted(cum, cum[-1] * np.arange(1, max(1, n_groups)) / max(1, n_groups), side="left") + 1
    edges = np.unique(np.concatenate([[0], np.minimum(cuts, z.size), [z.size]]))
    return [(int(a), int(b)) for a, b in zip(edges[:-1], edges[1:]) if b > a]



# PYAS_ZERO_SIGN_FALLBACK=warn: a query whose zero-sign pass the device cannot
# run returns the reduction with the device's sign of a zero min/max and a
# RuntimeWarning, instead of raising (the default keeps NumPy's bytes or fails)
_SIGN_FALLBACK_WARN = os.environ.get("PYAS_ZERO_SIGN_FALLBACK", "") == "warn"


def _axes_mask(axes):
    """The ABI's axes mask: bit d set for every reduced dim d."""
    mask = 0
    for a in axes:
        mask |= 1 << a
    return mask


def _grid_struct(ndim, axes, final_shape, tables, tbuf_ptr, offsets_ptr):
    """pyas_grid of a box query from ``_grid_from_dims``' tables, whose blob
    lies on the device at ``tbuf_ptr``: a kept dim gets its three position
    tables, a reduced dim extent 1 and none.  ``tbuf_ptr`` None (only
    ``tables["n_coords"]`` is read then) leaves every table NULL, for a launch
    that takes the chunk grid alone."""
    g = _lib.Grid()
    g.ndim = ndim
    g.axes_mask = _axes_mask(axes)
    for d in range(ndim):
        g.n_coords[d] = tables["n_coords"][d]
        g.out_extent[d] = final_shape[d] if d not in axes else 1
        if d not in axes and tbuf_ptr is not None:
            g.pos_coord[d] = tbuf_ptr + 4 * tables["pos_coord"][d]
            g.pos_local[d] = tbuf_ptr + 4 * tables["pos_local"][d]
            g.coord_count[d] = tbuf_ptr + 4 * tables["coord_count"][d]
    g.chunk_out_offsets = offsets_ptr
    return g


def _chunk_outputs(chunk_projs, axes, final_shape):
    """Where each chunk's partial outputs go.  ``chunk_projs``: per chunk, its
    per-dim projections.  Returns ``(out_off, f_all)``: chunk k's outputs (C
    order over its kept selected dims) are entries ``out_off[k]:out_off[k+1]``
    of ``f_all``, each the flat index of its final output."""
    sizes, fidx = [], []
    for projs in chunk_projs:
        pos = [np.asarray(p.out_pos, dtype=np.int64) if i not in axes else np.zeros(1, dtype=np.int64)
               for i, p in enumerate(projs)]
        grids = np.meshgrid(*pos, indexing="ij")
        fidx.append(np.ravel_multi_index([x.reshape(-1) for x in grids], final_shape))
        sizes.append(grids[0].size)
    out_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    return out_off, np.concatenate(fidx).astype(np.int64, copy=False)


def _segment_meta(chunk_projs, axes, final_shape):
    """Segments of a ``*_combine_segments`` call over the partial outputs of
    :func:`_chunk_outputs`: ``(out_off, order, seg)``, final output f
    combining the partial outputs ``order[seg[f]:seg[f+1]]``, in chunk order
    (a stable sort)."""
    out_off, f_all = _chunk_outputs(chunk_projs, axes, final_shape)
    order = np.argsort(f_all, kind="stable").astype(np.int64)
    seg = np.searchsorted(f_all[order], np.arange(int(np.prod(final_shape)) + 1)).astype(np.int64)
    return out_off, order, seg


def _fold_levels(n, seg=_RECORD_SEG):
    """The fold of ``n`` per-chunk records into one, in chunk order: groups of
    ``seg`` consecutive records per thread, level after level (a fixed
    function of the chunk count alone).  Returns ``(levels, n_rec)``: per
    level its segment count and segment bounds, and the records the per-chunk
    pass and every level but the last write."""
    levels, m = [], n
    while True:
        n_seg = -(-m // seg)
        levels.append((n_seg, np.minimum(np.arange(n_seg + 1, dtype=np.int64) * seg, m)))
        if n_seg == 1:
            break
        m = n_seg
    return levels, n + sum(n_seg for n_seg, _ in levels[:-1])


def _sign_fallback(err):
    """A zero-sign pass the device cannot run for this query (e.g. 2^31 or
    more reduced elements per output: its scan keys are 32-bit).  Raises
    ``err`` unless the caller opted in (PYAS_ZERO_SIGN_FALLBACK=warn): the
    reduction itself is complete, but the sign of a zero min/max would be the
    device reduction's rather than NumPy's (storage.py:99-100)."""
    if not _SIGN_FALLBACK_WARN:
        raise err
    warnings.warn(f"the sign of a zero min/max is not NumPy's for this query ({err})",
                  RuntimeWarning, stacklevel=3)

def _selection_position(index, bad, dim):
    """Global indices along a dimension (``bad``: the masked entries, whose
    index is 0 and whose position stays 0) as positions in its selection:
    ``dim`` is the dimension's indexer, a slice of step >= 1 or a strictly
    increasing index array."""
    if dim.kind == "slice":
        pos = index - dim.start if dim.start else index
        if dim.step != 1:
            pos = pos // dim.step
        if not dim.start:
            return pos                    # (the entries of ``bad`` are 0 already)
    else:
        pos = np.searchsorted(dim.sel, index).astype(np.int64)
    return np.where(bad, 0, pos)


class Active:
    """GPU-backed ``Active`` over one chunked variable."""

    def __new__(cls, *args, **kwargs):
        inst = super().__new__(cls)
        inst._methods = {"min": np.ma.min, "max": np.ma.max, "sum": np.ma.sum, "mean": np.ma.sum,
                         "var": np.ma.var, "std": np.ma.std}
        return inst

    def __init__(self, dataset, ncvar=None, axis=None, interface_type=None, max_threads: int = 30,
                 storage_options=None, active_storage_url=None, option_disable_chunk_cache=False,
                 *, device: int = 0, device_inflate="auto", group=None, resident: bool = False):
        """``dataset``: a netCDF4/HDF5 file path with ``ncvar`` naming the
        variable (``active.py:185-280``: same signature, checks and errors),
        or a :class:`ChunkedVariable` (the reference accepts a pyfive
        Dataset).  Local files only: ``interface_type`` "s3"/"https" and
        ``storage_options`` (remote object stores) are not served here."""
        if interface_type not in (None, "", "posix", "ActivePosix") or storage_options is not None:
            raise NotImplementedError(
                f"interface_type={interface_type!r}: remote object stores are outside this backend; "
                "point Reductionist clients at pyactivestorage_amd.reductionist_server instead")
        self.active_storage_url = active_storage_url
        self.option_disable_chunk_cache = bool(option_disable_chunk_cache)
        if dataset is None:
            raise ValueError(f"Must use a valid file name or variable object for dataset. Got {dataset!r}")
        if isinstance(dataset, (str, os.PathLike)):
            path = os.fspath(dataset)
            if not os.path.isfile(path):
                raise ValueError(f"Must use existing file for uri. {path} not found")
            if ncvar is None:
                raise ValueError("Must set a netCDF variable name to slice")
            from .hdf5 import open_variable
            variable = open_variable(path, ncvar)
        elif isinstance(dataset, ChunkedVariable):
            variable = dataset
        else:
            raise TypeError(f"Variable object dataset can only be a ChunkedVariable. Got {dataset!r}")
        self.uri = dataset
        self.ncvar = ncvar
        self.ds = variable
        if axis is not None:
            axis = (axis,) if isinstance(axis, int) else tuple(axis)
        self._axis = axis
        self._components = False
        self._method = None
        self._ddof = 0                  # var / std: the divisor is count - ddof
        self._weights = None            # mean / sum: {dim: float64 vector} of the next query
        self._mweights = None           # var / std / cov / corr: the weights= keyword of the next query
        self._hist = None               # histogram: the bins of the next query (_check_hist)
        self._quant = None              # quantile: {"q": float64 (0-D or 1-D), "method": str} of the next query
        self._co = None                 # cov / corr: the second variable's Active of the next query
        self._trend = None              # trend: {"along": dim >= 0, "coord": float64 vector} of the next query
        self._trend_path = None         # the last trend query: "cols" (dense column kernel) or "walk"
        self._grouped = None            # grouped: {"stat", "along", "labels", "n_groups"} of the next query
        self._grouped_path = None       # the last grouped query: "cols" (dense column kernel) or "walk"
        self._spell = None              # spell: {"along", "op", "threshold", "stat", "min_length"} of the next query
        self._spell_path = None         # the last spell query: "cols" (dense column kernel) or "walk"
        self._rolling = None            # rolling: {"along", "window", "stat", "which"} of the next query
        self._rolling_path = None       # the last rolling query: "cols" (dense column kernel) or "walk"
        self._argext = None             # argmax / argmin: {"along", "which", "name"} of the next query
        self._argext_path = None        # the last argmax / argmin query: "cols" (dense column kernel) or "walk"
        self._exceed = None             # exceed: {"op", "threshold", "stat"} of the next query
        self._exceed_path = None        # the last exceed query: "cols" (dense column kernel) or "walk"
        self._select_stats = None       # the last quantile query: its digit width, count launches and chains
        self._max_threads = int(max_threads)
        self.device = device
        # f3: zlib chunks inflate on the GPU (True), on the host reader threads
        # straight into the pinned ring (False), or whichever is faster for the
        # query's stream count ("auto", inflate_on_device)
        if device_inflate not in (True, False, "auto"):
            raise ValueError(f"device_inflate must be True, False or 'auto'. Got {device_inflate!r}")
        self.device_inflate = device_inflate
        # row (e): a torch.distributed process group (one process per GPU).
        # Each rank reads and reduces a contiguous range of the query's chunks
        # from its own GPU; one all-gather of the per-rank partial grids and a
        # fixed rank-order device combine give every rank the same result.
        self.group = group
        # keep the variable's decoded chunks in HBM across queries (288 GB per
        # MI355X): later queries read only chunks not loaded yet
        self.resident = bool(resident)
        self.missing = None
        self.data_read = 0
        self._held = threading.local()

    # -- API mirrored from active.py:355-418 ------------------------------
    @property
    def components(self):
        return self._components

    @components.setter
    def components(self, value):
        self._components = bool(value)

    @property
    def method(self):
        return self._methods.get(self._method)

    @method.setter
    def method(self, value):
        if value is not None and value not in self._methods:
            raise ValueError(f"Bad 'method': {value}. Choose from min/max/mean/sum.")
        self._method = value
        self._ddof = 0
        self._weights = None
        self._mweights = None
        self._hist = None
        self._quant = None
        self._co = None
        self._trend = None
        self._grouped = None
        self._spell = None
        self._rolling = None
        self._argext = None
        self._exceed = None

    @property
    def rolling_path(self):
        """Which kernel the last :meth:`rolling` query ran: ``"cols"`` (the
        dense column walk, pyas_roll_cols) or ``"walk"`` (the per-element walk,
        pyas_roll_axes); None before the first one and after a query that
        reached no kernel (an empty selection)."""
        return self._rolling_path

    @property
    def exceed_path(self):
        """Which kernel the last :meth:`exceed` query ran: ``"cols"`` (the dense
        column walk, pyas_exceed_cols) or ``"walk"`` (pyas_exceed_axes: the
        per-element walk, or the tile kernel when every dim is reduced); None
        before the first one and after a query that reached no kernel (an
        empty selection)."""
        return self._exceed_path

    @property
    def argext_path(self):
        """Which kernel the last :meth:`argmax` / :meth:`argmin` query ran:
        ``"cols"`` (the dense column walk, pyas_argext_cols) or ``"walk"``
        (the per-element walk, pyas_argext_axes); None before the first one
        and after a query that reached no kernel (an empty selection)."""
        return self._argext_path

    @property
    def spell_path(self):
        """Which kernel the last :meth:`spell` query ran: ``"cols"`` (the dense
        column walk, pyas_spell_cols) or ``"walk"`` (the per-element walk,
        pyas_spell_axes); None before the first one and after a query that
        reached no kernel (an empty selection)."""
        return self._spell_path

    @property
    def grouped_path(self):
        """Which kernel the last :meth:`grouped` query ran: ``"cols"`` (the
        dense column walk, pyas_group_cols) or ``"walk"`` (the per-element
        walk, pyas_group_axes); None before the first one and after a query
        that reached no kernel (an empty selection, no group)."""
        return self._grouped_path

    @property
    def trend_path(self):
        """Which kernel the last :meth:`trend` query ran: ``"cols"`` (the dense
        column walk, pyas_trend_cols) or ``"walk"`` (the per-element walk,
        pyas_trend_axes); None before the first one and after a query that
        reached no kernel (an empty selection)."""
        return self._trend_path

    @property
    def weights(self):
        """The weights of the next :meth:`mean` / :meth:`sum` query (``{dim:
        float64 vector}``) or None.  The property belongs to those two: a
        :meth:`var`, :meth:`std`, :meth:`cov` or :meth:`corr` query takes its
        weights through its own ``weights=`` keyword and refuses the property."""
        return self._weights

    @weights.setter
    def weights(self, value):
        self._weights = self._check_weights(value)

    def _check_weights(self, weights):
        """``{dim: 1-D array-like}`` as ``{dim >= 0: float64 vector}``: each
        vector has ``shape[dim]`` entries (it is indexed by the global index
        along ``dim``), all finite and >= 0.  ValueError otherwise."""
        if weights is None:
            return None
        if not hasattr(weights, "items"):
            raise ValueError("weights must be a mapping {dim: 1-D array-like}")
        ndim, shape = self.ds.ndim, self.ds.shape
        out = {}
        for dim, w in weights.items():
            if isinstance(dim, (bool, np.bool_)) or not isinstance(dim, (int, np.integer)) or not -ndim <= dim < ndim:
                raise ValueError(f"weights: dimension {dim!r} is out of range for {ndim} dimensions")
            d = int(dim) % ndim
            if d in out:
                raise ValueError(f"weights: dimension {d} is given twice")
            try:
                w = np.asarray(w, dtype=np.float64)
            except (TypeError, ValueError) as exc:
                raise ValueError(f"weights[{dim!r}] is not numeric: {exc}") from None
            if w.ndim != 1 or w.size != shape[d]:
                raise ValueError(f"weights[{dim!r}] must be 1-D with {shape[d]} entries. Got shape {w.shape}")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError(f"weights[{dim!r}] has a negative, NaN or infinite entry")
            out[d] = w
        return out

    def mean(self, axis=None, weights=None):
        """Mean of the unmasked elements.  With ``weights = {dim: vector}`` the
        weighted mean ``sum(w x) / sum(w)`` in float64, where an element's
        weight is the product of its dims' entries (dims not named: 1),
        multiplied in ascending dim order.  The result is masked where
        ``sum(w) == 0``: no unmasked element, or every unmasked element has
        weight exactly 0 (``np.ma.average`` gives NaN for such a full
        reduction; here it is masked).  With ``components`` the result is
        ``{"sum": sum(w x), "sum_of_weights": sum(w), "n": count}``."""
        if weights is not None:
            self._weights = self._check_weights(weights)
        self._method = "mean"
        if axis is not None:
            self._axis = axis
        return self

    def min(self, axis=None):
        self._method = "min"
        if axis is not None:
            self._axis = axis
        return self

    def max(self, axis=None):
        self._method = "max"
        if axis is not None:
            self._axis = axis
        return self

    def sum(self, axis=None, weights=None):
        """Sum of the unmasked elements; with ``weights`` (see :meth:`mean`)
        the weighted sum ``sum(w x)`` in float64, masked where no element is
        unmasked.  With ``components``: ``{"sum": sum(w x), "n": count}``."""
        if weights is not None:
            self._weights = self._check_weights(weights)
        self._method = "sum"
        if axis is not None:
            self._axis = axis
        return self

    def var(self, axis=None, ddof=0, weights=None):
        """Variance of the unmasked elements, ``m2 / (count - ddof)`` in
        float64 (``np.ma.var`` of the float64 selection), masked where
        ``count - ddof <= 0``.  One pass on the device (pyas_moments_axes).

        With ``weights = {dim: vector}`` (the mapping :meth:`mean` takes; the
        ``weights`` property belongs to :meth:`mean` / :meth:`sum` and is
        refused here) the weighted variance ``m2 / fact`` in float64:
        ``m2 = sum w (x - mean)^2`` about the weighted mean, and
        ``fact = (sw sw - ddof sw2) / sw`` with ``sw = sum w``,
        ``sw2 = sum w^2``, the normaliser of ``np.cov(aweights=w, ddof=ddof)``.
        Masked where ``sw == 0`` or ``sw sw - ddof sw2 <= 0``; a counted NaN or
        infinity gives NaN at any weight, exactly 0 included.  One pass on the
        device (pyas_wcomoments_axes).  With ``components`` the result is a
        dict of ``mean``, ``m2``, ``n``, ``sum_of_weights`` and
        ``sum_of_weights2``; ``wmoments.merge`` combines the records of
        disjoint selections.  The keyword holds for one query."""
        return self._set_moments("var", axis, ddof, weights)

    def std(self, axis=None, ddof=0, weights=None):
        """Standard deviation: the square root of :meth:`var`."""
        return self._set_moments("std", axis, ddof, weights)

    def cov(self, other, axis=None, ddof=0, weights=None):
        """Covariance with ``other``, an ``Active`` over a second variable of
        the same shape, chunks and dtype (byte order and filters may differ;
        it may be this object): ``cxy / (n - ddof)`` in float64 over the pairs
        selected and unmasked in both variables, each side under its own
        missing-data attributes; ``np.cov(xs, ys, ddof=ddof)[0, 1]`` of the
        compressed float64 pairs.  Masked where ``n - ddof <= 0``; NaN where a
        counted pair holds a NaN or an infinity.  One pass on the device over
        both variables' chunks (pyas_comoments_axes).  With ``components`` the
        result is a dict of ``n``, ``mean_x``, ``mean_y``,
        ``m2_x = sum (x - mean_x)^2``, ``m2_y`` and
        ``cxy = sum (x - mean_x)(y - mean_y)``: the slope of the regression of
        ``other`` on this variable is ``cxy / m2_x``, and
        ``comoments.merge`` combines the components of disjoint selections.
        The settings hold for one query.

        With ``weights`` (see :meth:`var`) the weighted covariance
        ``cxy / fact`` with ``cxy = sum w (x - mean_x)(y - mean_y)`` about the
        weighted means: ``np.cov(xs, ys, aweights=w, ddof=ddof)[0, 1]``,
        masked as the weighted :meth:`var` (pyas_wcomoments_axes).  The
        components then also hold ``sum_of_weights`` and
        ``sum_of_weights2``."""
        return self._set_comoments("cov", other, axis, ddof, weights)

    def corr(self, other, axis=None, weights=None):
        """Pearson's correlation with ``other`` (see :meth:`cov`):
        ``cxy / sqrt(m2_x) / sqrt(m2_y)`` clipped to [-1, 1] as
        ``np.corrcoef`` clips.  Masked where no pair is counted; NaN, not
        masked, where either variable is constant over the counted pairs.
        With ``weights`` (see :meth:`var`) the weighted centred correlation
        (the pattern correlation of two fields under area weights), masked
        where ``sum w == 0``."""
        return self._set_comoments("corr", other, axis, 0, weights)

    def trend(self, along, coord=None, axis=None):
        """The least-squares slope of the data against a coordinate, per
        output: with ``x = coord[i]`` for an element at global index ``i``
        along dimension ``along`` and ``y`` its value as float64,
        ``slope = cxy / m2_x`` over the selected unmasked elements
        (``cxy = sum (x - mean_x)(y - mean_y)``, ``m2_x = sum (x - mean_x)^2``),
        one pass on the device.  ``along``: an int in ``[-ndim, ndim)`` that
        must be among the reduced axes; ``coord``: 1-D, ``shape[along]`` finite
        entries (they may repeat and need not be monotonic), ``None`` meaning
        ``arange(shape[along])``.  The query returns a float64 masked array of
        ``final_shape``: masked where no element counts; NaN, not masked,
        where ``m2_x == 0`` (one counted element, or all counted coordinates
        equal) and where a counted value is NaN or infinite; exactly 0 for
        constant data.  With ``components`` a dict of ``slope``, ``intercept``
        (``mean_y - slope mean_x``), ``n``, ``mean_x``, ``mean_y``, ``m2_x``,
        ``m2_y`` and ``cxy``: the fields of a :meth:`cov` record with the
        coordinate as ``x``, so ``comoments.merge`` combines the components of
        disjoint selections.  A unit-step box query whose reduced axes are a
        leading prefix of the dims (``along=0, axis=(0,)``) runs the dense
        column kernel (pyas_trend_cols), anything else the per-element walk
        (pyas_trend_axes): see :attr:`trend_path`.  The settings hold for one
        query."""
        ndim = self.ds.ndim
        if isinstance(along, (bool, np.bool_)) or not isinstance(along, (int, np.integer)) \
                or not -ndim <= along < ndim:
            raise ValueError(f"trend: along={along!r} is out of range for {ndim} dimensions")
        d = int(along) % ndim
        self._trend = {"along": d, "coord": trend.check_coord(coord, self.ds.shape[d])}
        self._method = "trend"
        if axis is not None:
            self._axis = axis
        return self

    def spell(self, along, op, threshold, stat="longest", min_length=1):
        """Spells past a threshold along one dimension, per output, in one
        pass on the device.  An element is *true* when it is selected,
        unmasked and ``float64(x) op threshold`` holds (``op``: ``"gt"``,
        ``"ge"``, ``"lt"`` or ``"le"``; ``threshold``: a finite number; a NaN
        compares false but counts as unmasked; a masked element is false).  A
        run is a maximal sequence of true elements that are consecutive in the
        selection along ``along`` (with ``[::3]``, consecutive selected
        elements).  ``stat``: ``"longest"``, the longest run (CDD, CWD);
        ``"days"``, the total length of the runs of at least ``min_length``
        (WSDI, CSDI); ``"events"``, the number of such runs.  ``along``: an
        int in ``[-ndim, ndim)``; it becomes the only reduced axis, so the
        query returns an int64 masked array of the shape
        ``mean(axis=(along,))`` returns, masked where an output has no
        unmasked element.  With ``components`` a dict of the record's fields
        (``n``, ``n_true``, ``len``, ``head``, ``tail``, ``best``, ``days``,
        ``events``, ``min_length``: see :mod:`.spell`) and ``longest``,
        ``days_total`` and ``events_total`` finalized, so ``spell.merge`` joins
        the components of selections that follow each other along ``along``
        (years, files) and ``spell.finalize`` reads the result.  The selection
        along ``along`` must be a slice of step >= 1, a strictly increasing
        index list or a boolean mask (ValueError otherwise) of fewer than 2^31
        positions.  A unit-step box query with ``along=0`` and a dimension
        behind it runs the dense column kernel (pyas_spell_cols), anything
        else the per-element walk (pyas_spell_axes): see :attr:`spell_path`;
        both give the same integers.  The settings hold for one query."""
        ndim = self.ds.ndim
        if isinstance(along, (bool, np.bool_)) or not isinstance(along, (int, np.integer)) \
                or not -ndim <= along < ndim:
            raise ValueError(f"spell: along={along!r} is out of range for {ndim} dimensions")
        d = int(along) % ndim
        try:
            settings = {"along": d, "op": spell.check_op(op), "threshold": spell.check_threshold(threshold),
                        "stat": spell.check_stat(stat), "min_length": spell.check_min_length(min_length)}
        except ValueError as exc:
            raise ValueError(f"spell: {exc}") from None
        self._spell = settings
        self._method = "spell"
        self._axis = (d,)
        return self

    def rolling(self, along, window, stat="sum", extreme="max"):
        """The extreme running-window sum or mean along one dimension, per
        output, in one pass on the device: Rx5day is
        ``a.rolling(0, 5)[index]``, the hottest 3-day mean
        ``a.rolling(0, 3, stat="mean")[index]``.  A *window* is ``window``
        elements consecutive in the selection along ``along`` (with ``[::3]``,
        every third element joins).  It is *valid* when all of its elements
        are unmasked under ``_FillValue``, ``missing_value``, ``valid_min``
        and ``valid_max``: a window with a missing day gives no value (a NaN
        is data, not a missing day).  A valid window's sum is
        ``s = f64(x[p]); s += f64(x[p+1]); ...; s += f64(x[p+w-1])``: every
        element converts as ``astype(float64)`` does and the ``w - 1``
        additions are float64, oldest element first.  This order is the
        definition (no running add-and-subtract), so every path gives the
        same bits.  The result is the largest (``extreme="max"``) or smallest
        (``"min"``) valid window sum as float64; ``stat="mean"`` divides that
        sum once by ``float64(window)`` (division by a positive constant is
        monotone, so this is the extreme of the means).  A NaN sum (a NaN
        element, or ``+inf`` and ``-inf`` in one window) propagates as in
        ``np.max`` / ``np.min``: the first window whose sum is NaN wins.
        Among equal sums the first window wins; ``-0.0 == +0.0``.  ``along``:
        an int in ``[-ndim, ndim)``, the only reduced axis, kept with extent
        1; ``window``: an int in ``1 .. 8`` (NotImplementedError beyond,
        ValueError for anything that is not an int >= 1).  The result is
        masked where an output has no valid window: fewer than ``window``
        selected positions, or a masked element in every window.  With
        ``components`` a dict of ``value`` (the result), ``sum`` (the extreme
        window sum), ``position`` (int64, the position in the selection of
        the winning window's first element, masked like ``value``),
        ``n_windows`` (valid windows), ``n`` (unmasked positions), ``len``
        (positions) and the record's other fields (``best``, ``window``,
        ``which``, ``head``, ``tail``, ``head_ok``, ``tail_ok``: see
        :mod:`.rolling`), so ``rolling.merge`` joins the components of
        selections that follow each other along ``along`` (years, files)
        with the windows across the join, and ``rolling.finalize`` reads the
        result.  The selection along ``along`` must be a slice of step >= 1,
        a strictly increasing index list or a boolean mask (ValueError
        otherwise) of fewer than 2^31 positions.  A unit-step box query with
        ``along=0`` and a dimension behind it runs the dense column kernel
        (pyas_roll_cols), anything else the per-element walk
        (pyas_roll_axes): see :attr:`rolling_path`; both give the same
        records byte for byte.  The settings hold for one query."""
        ndim = self.ds.ndim
        if isinstance(along, (bool, np.bool_)) or not isinstance(along, (int, np.integer)) \
                or not -ndim <= along < ndim:
            raise ValueError(f"rolling: along={along!r} is out of range for {ndim} dimensions")
        d = int(along) % ndim
        try:
            settings = {"along": d, "window": rolling.check_window(window), "stat": rolling.check_stat(stat),
                        "which": rolling.check_extreme(extreme)}
        except ValueError as exc:
            raise ValueError(f"rolling: {exc}") from None
        except NotImplementedError as exc:
            raise NotImplementedError(f"rolling: {exc}") from None
        self._rolling = settings
        self._method = "rolling"
        self._axis = (d,)
        return self

    def argmax(self, along):
        """Where the maximum lies along one dimension, per output, in one pass
        on the device: ``a.argmax(0)[index]`` is the position in the selection
        along ``along`` of the largest unmasked element, what
        ``np.argmax(data[index], axis=along)`` gives for unmasked data, as an
        int64 masked array of the selection's shape with ``along`` kept at
        extent 1, masked where an output has no unmasked element.  Masked
        elements (``_FillValue``, ``missing_value``, ``valid_min``,
        ``valid_max``) never win; among elements equal to the extreme the
        first position wins; ``-0.0`` and ``+0.0`` are equal; if an unmasked
        element is a NaN the first unmasked NaN wins, as in NumPy; values are
        compared in the variable's own type (8-byte integers exactly).
        ``along``: an int in ``[-ndim, ndim)``, the only reduced axis.  The
        selection along ``along`` must be a slice of step >= 1, a strictly
        increasing index list or a boolean mask (ValueError otherwise) of
        fewer than 2^31 positions; any hyperslab on the other dims.  With
        ``components`` a dict of ``position`` (the result), ``index`` (the
        global index along ``along`` in the variable, int64), ``value`` (the
        winning element itself, bit for bit, in the variable's dtype, masked
        like the result) and ``n`` (the count of unmasked elements, int64,
        never masked); ``argext.merge`` joins the components of selections
        that lie along ``along`` (years, files).  ``value`` is the element at
        ``index``: the sign of a zero is that element's, so it may differ from
        :attr:`method` ``"max"`` / ``"min"``, which follow NumPy's tie rule
        for zeros of both signs.  A unit-step box query with
        ``along=0`` and a dimension behind it runs the dense column kernel
        (pyas_argext_cols), anything else the per-element walk
        (pyas_argext_axes): see :attr:`argext_path`; both give the same
        records.  The setting holds for one query."""
        return self._set_argext("argmax", along, "max")

    def argmin(self, along):
        """Where the minimum lies along one dimension: :meth:`argmax` with
        the smallest unmasked element as the winner.  A NaN still wins over
        every number (the first unmasked NaN), as in ``np.argmin``."""
        return self._set_argext("argmin", along, "min")

    def _set_argext(self, name, along, which):
        try:
            d = argext.check_along(along, self.ds.ndim)
        except ValueError as exc:
            raise ValueError(f"{name}: {exc}") from None
        self._argext = {"along": d, "which": which, "name": name}
        self._method = name
        self._axis = (d,)
        return self

    def exceed(self, op, threshold, stat="count", axis=None):
        """Counts, sums and degree days past a threshold, per output, in one
        pass on the device (frost and summer days, R10mm, PRCPTOT, SDII,
        R95pTOT, TX90p, heating and cooling degree days).  An element is
        *true* when it is selected, unmasked and ``float64(x) op threshold``
        holds (``op``: ``"gt"``, ``"ge"``, ``"lt"`` or ``"le"``; a NaN compares
        false but counts as unmasked; a masked element is never true).  Every
        element converts as ``astype(float64)`` does, so 8-byte integers
        compare as their float64 conversion: ``2**53 + 1`` is not ``gt``
        ``2**53``.  ``axis``: any subset of the dims, as for :meth:`var`.
        ``threshold`` is a finite real scalar, or a per-output field:
        array-like with ``ndim`` dims whose extent is ``shape[d]`` on every
        kept dim and 1 on every reduced one, converted to float64 and indexed
        by *global* index (like ``weights``, ``coord`` and ``labels``), so
        slices, steps, index lists and boolean masks on the kept dims pick the
        matching thresholds; a full-variable ``a.quantile(q, axis=axes)[...]``
        is a valid field for ``axis=axes`` as it stands.  A field must be
        finite everywhere except at the masked entries of a masked array:
        nothing compares true there and the result is masked there.  A field
        with every dim reduced has one entry and is the scalar case.
        ValueError for a wrong rank or shape.  ``stat``: ``"count"``, the
        number of true elements (int64); ``"fraction"``, ``n_true / n``;
        ``"sum"``, the sum of the true elements in float64 from the first
        addition (0.0 when nothing is true); ``"mean"``, ``sum / n_true``;
        ``"excess"``, the sum over the true elements of ``|x - threshold|``,
        each term one float64 subtraction (``x - t`` for ``gt`` / ``ge``,
        ``t - x`` for ``lt`` / ``le``) added in float64, never derived from
        ``sum - t n_true``.  The query returns a masked array of
        ``final_shape`` (reduced dims kept at extent 1), float64 except
        ``count``, masked where the output has no unmasked element (``mean``:
        no true element) and where its threshold is masked.  With
        ``components`` a dict of ``n``, ``n_true`` (int64), ``sum`` and
        ``excess`` (float64), none of them masked (``n_true == 0`` where the
        threshold is masked); ``exceed.merge`` adds the components of
        disjoint selections (years, files) and assumes the same ``op`` and
        the same threshold on both sides, and ``exceed.finalize`` reads a
        result from them.  A unit-step box query whose reduced axes are a
        leading prefix of the dims (``axis=(0,)``) runs the dense column
        kernel (pyas_exceed_cols), anything else pyas_exceed_axes: see
        :attr:`exceed_path`; both give the same ``n`` and ``n_true``, and
        sums that may differ in the last bits.  The settings hold for one
        query."""
        before = self._axis
        try:
            op, stat = spell.check_op(op), exceed.check_stat(stat)
            if axis is not None:
                self._axis = axis
            if self._axis is None:
                axes = tuple(range(self.ds.ndim))
            else:
                if isinstance(self._axis, int):
                    self._axis = (self._axis,)
                axes = self._norm_axes()
            field = exceed.check_field(threshold, self.ds.shape, axes)
        except ValueError as exc:
            self._axis = before
            raise ValueError(f"exceed: {exc}") from None
        self._exceed = {"op": op, "stat": stat, "field": field, "axes": axes}
        self._method = "exceed"
        return self

    def grouped(self, stat, along, labels, axis=None, ddof=0, n_groups=None):
        """One statistic per label along a reduced dimension, in one pass on
        the device: ``stat`` (``"mean"``, ``"var"``, ``"std"``, ``"count"``,
        ``"min"``, ``"max"`` or ``"sum"``) of the selected unmasked elements whose global index ``i`` along
        dimension ``along`` has ``labels[i] == g``, for every group ``g`` in
        ``range(G)``: a monthly climatology with ``labels`` the month of each
        time step.  ``along``: an int in ``[-ndim, ndim)`` that must be among
        the reduced axes; ``labels``: 1-D, ``shape[along]`` integers, a
        negative one putting its index in no group (on the dense path such
        rows are not read); ``n_groups``: ``G``, None meaning
        ``max(labels) + 1`` (0 when every label is negative); ``ddof``: as for
        :meth:`var` (``mean`` and ``count`` ignore it).  The query returns an
        array of ``final_shape`` with ``G`` in place of the 1 along ``along``:
        for ``mean``, ``var`` and ``std`` a float64 masked array (``mean``
        masked where the group counts no element, ``var`` / ``std`` where
        ``count - ddof <= 0``; NaN where a counted value is NaN or infinite),
        for ``count`` an int64 ``ndarray``.  An element's value is its float64
        conversion, as for :meth:`var`.  With ``components`` a dict of
        ``mean``, ``m2`` and ``n`` as :meth:`var` returns them, so
        ``moments.merge`` combines the components of disjoint selections.
        ``min`` / ``max`` / ``sum`` (``ddof`` ignored) always return a masked
        array with a full mask, masked where the group counts no element:
        ``min`` and ``max`` in the variable's dtype (native byte order),
        compared in that type (8-byte integers stay exact), NaN where the
        group counts a NaN as ``np.ma.min`` gives it, the sign of a zero
        extreme not specified; ``sum`` in ``dtypes.sum_dtype``: int64 / uint64
        wrapping modulo 2^64 as NumPy's sums, floats added in float64 from
        the first element and rounded once for a float32 variable.  Their
        ``components`` are ``sum`` (float64, int64 or uint64), ``min``,
        ``max`` (the variable's dtype) and ``n``, and
        ``grouped.merge_partials`` combines the records of disjoint
        selections.  A unit-step box query whose reduced axes are a leading
        prefix of the dims (``along=0, axis=(0,)``) runs the dense column
        kernel (pyas_group_cols, pyas_group_cols_partial for min / max /
        sum), anything else the per-element walk (pyas_group_axes,
        pyas_group_axes_partial): see :attr:`grouped_path`.  The settings
        hold for one query."""
        if stat not in grouped.STATS:
            raise ValueError(f"grouped: stat must be one of {grouped.STATS}. Got {stat!r}")
        ndim = self.ds.ndim
        if isinstance(along, (bool, np.bool_)) or not isinstance(along, (int, np.integer)) \
                or not -ndim <= along < ndim:
            raise ValueError(f"grouped: along={along!r} is out of range for {ndim} dimensions")
        d = int(along) % ndim
        lab, n_g = grouped.check_labels(labels, self.ds.shape[d], n_groups)
        self._set_moments("grouped", axis, ddof)
        self._grouped = {"stat": stat, "along": d, "labels": lab, "n_groups": n_g}
        return self

    def histogram(self, bins=10, range=None, axis=None):   # noqa: A002 - NumPy's argument name
        """Binned counts of the unmasked elements, one pass on the device
        (pyas_hist_axes).  Each element converts to float64 as
        ``astype(float64)`` does; bin ``i`` holds ``e[i] <= x < e[i+1]`` and the
        last bin also ``x == e[n]``: ``np.histogram`` of the float64 selection.
        ``bins``: an int ``n >= 1`` (edges ``np.linspace(lo, hi, n + 1)`` over
        ``range = (lo, hi)``; ``range=None`` takes the selection's unmasked
        min and max, ``(0, 1)`` when nothing is unmasked) or a sequence of
        finite, strictly increasing edges.  The query returns an int64
        ``ndarray`` of shape ``final_shape + (n_bins,)`` (never masked); with
        ``components`` a dict of ``counts``, ``bin_edges``, ``n`` (the unmasked
        count), ``below``, ``above`` and ``nan``.  The settings hold for one
        query."""
        self._hist = self._check_hist(bins, range)
        self._method = "histogram"
        if axis is not None:
            self._axis = axis
        return self

    def quantile(self, q, axis=None, method="linear"):
        """Exact quantiles of the unmasked elements: per output
        ``np.quantile(x64, q, method=method)`` of the float64 copy ``x64`` of
        its unmasked selected elements, found on the device by a radix select
        over order-preserving keys (pyas_select_axes / pyas_select_step), so
        no element is sorted or copied.  ``q``: a scalar or 1-D sequence in
        [0, 1]; ``method``: ``linear``, ``lower``, ``higher``, ``midpoint`` or
        ``nearest``, with NumPy's meaning.  The query returns a float64 masked
        array of shape ``final_shape + q.shape``: masked where an output has
        no unmasked element, NaN where any of its unmasked elements is NaN.
        With ``components`` a dict of ``quantile``, ``n`` (int64: the unmasked
        elements per output, NaNs included) and ``nan`` (int64).  The sign of
        a zero result is not specified.  The settings hold for one query."""
        self._quant = {"q": quantile.check_q(q), "method": quantile.check_method(method)}
        self._method = "quantile"
        if axis is not None:
            self._axis = axis
        return self

    def median(self, axis=None):
        """The median of the unmasked elements: :meth:`quantile` at 0.5."""
        return self.quantile(0.5, axis=axis)

    @staticmethod
    def _check_hist(bins, range_):
        """``{"n": bins, "edges": float64 edges or None (range=None: found by
        the query), "uniform": evenly spaced}``.  ValueError for bad bins or
        range (histogram.edges)."""
        if histogram.is_count(bins):
            if range_ is None:
                histogram.edges(bins, (0.0, 1.0))     # the checks of the bin count
                return {"n": int(bins), "edges": None, "uniform": True}
            return {"n": int(bins), "edges": histogram.edges(bins, range_), "uniform": True}
        e = histogram.edges(bins)
        return {"n": e.size - 1, "edges": e, "uniform": False}

    def _set_moments(self, method, axis, ddof, weights=None):
        if isinstance(ddof, (bool, np.bool_)) or not isinstance(ddof, (int, np.integer)) or ddof < 0:
            raise ValueError(f"ddof must be a non-negative int. Got {ddof!r}")
        mweights = self._check_weights(weights)
        self._method = method
        self._ddof = int(ddof)
        self._mweights = mweights
        if axis is not None:
            self._axis = axis
        return self

    def _set_comoments(self, method, other, axis, ddof, weights=None):
        if not isinstance(other, Active):
            raise TypeError(f"{method}: other must be an Active over the second variable. Got {other!r}")
        x, y = self.ds, other.ds
        if tuple(x.shape) != tuple(y.shape) or tuple(x.chunks) != tuple(y.chunks):
            raise ValueError(f"{method}: the two variables must agree in shape and chunk shape. Got shape "
                             f"{tuple(x.shape)} in chunks {tuple(x.chunks)} and shape {tuple(y.shape)} in chunks "
                             f"{tuple(y.chunks)}")
        if x.dtype.kind != y.dtype.kind or x.dtype.itemsize != y.dtype.itemsize:
            raise NotImplementedError(f"{method}: the two variables must have the same dtype up to byte order. "
                                      f"Got {x.dtype.str} and {y.dtype.str}")
        if other.device != self.device:
            raise ValueError(f"{method}: the two Active objects are on devices {self.device} and {other.device}")
        self._set_moments(method, axis, ddof, weights)
        self._co = other
        return self

    # -- query -------------------------------------------------------------
    def __getitem__(self, index):
        self.missing = get_missing_attributes(self.ds.attrs)
        self.data_read = 0
        held = self._held.stores = []    # resident stores this query uses (this thread)
        try:
            return self._get_selection(index)
        finally:
            self._method = None          # active.py:633
            self._weights = None         # weights are per query
            self._mweights = None        # and so is a second-moment query's weights= keyword
            self._hist = None            # and so are a histogram's bins
            self._quant = None           # and a quantile's q and method
            self._co = None              # and a cov / corr's second variable
            self._trend = None           # and a trend's coordinate
            self._grouped = None         # and a grouped query's labels
            self._spell = None           # and a spell's threshold
            self._rolling = None         # and a rolling query's window
            self._argext = None          # and an arg-extreme's dimension
            self._exceed = None          # and an exceed query's threshold
            for store in held:
                _unhold(store)
            self._held.stores = []

    def _get_selection(self, index):
        ds = self.ds
        second = self._method in ("var", "std")
        if second and self.group is not None:
            raise NotImplementedError("var/std with group=…: second moments are reduced on one GPU only")
        has_w = self._weights is not None
        if has_w and self._method not in ("mean", "sum"):
            raise ValueError(f"weights apply to mean and sum only, not to method {self._method!r}")
        if has_w and self.group is not None:
            raise NotImplementedError("weights with group=…: weighted sums are reduced on one GPU only")
        hist = self._method == "histogram"
        if hist and self.group is not None:
            raise NotImplementedError("histogram with group=…: binned counts are reduced on one GPU only")
        quant = self._method == "quantile"
        if quant and self.group is not None:
            raise NotImplementedError("quantile with group=…: order statistics are selected on one GPU only")
        co = self._method in ("cov", "corr")
        if co and (self.group is not None or self._co.group is not None):
            raise NotImplementedError("cov/corr with group=…: co-moments are reduced on one GPU only")
        tr = self._method == "trend"
        if tr and self.group is not None:
            raise NotImplementedError("trend with group=…: co-moments are reduced on one GPU only")
        gr = self._method == "grouped"
        if gr and self.group is not None:
            raise NotImplementedError("grouped with group=…: second moments are reduced on one GPU only")
        sp = self._method == "spell"
        if sp and self.group is not None:
            raise NotImplementedError("spell with group=…: spell records are reduced on one GPU only")
        ro = self._method == "rolling"
        if ro and self.group is not None:
            raise NotImplementedError("rolling with group=…: running-window records are reduced on one GPU only")
        ax = self._method in ("argmax", "argmin")
        if ax and self.group is not None:
            raise NotImplementedError(f"{self._method} with group=…: arg-extreme records are reduced on one GPU only")
        ex = self._method == "exceed"
        if ex and self.group is not None:
            raise NotImplementedError("exceed with group=…: exceed records are reduced on one GPU only")
        if self._axis is None:
            self._axis = tuple(range(ds.ndim))
        elif isinstance(self._axis, int):
            self._axis = (self._axis,)
        if tr and self._trend["along"] not in self._norm_axes():
            raise ValueError(f"trend: along={self._trend['along']} is not among the reduced axes "
                             f"{self._norm_axes()}: the coordinate would be constant per output")
        if gr and self._grouped["along"] not in self._norm_axes():
            raise ValueError(f"grouped: along={self._grouped['along']} is not among the reduced axes "
                             f"{self._norm_axes()}: every output would hold one label")
        cache_key = None
        # (var / std, weighted, histogram, quantile, cov / corr, trend, grouped, spell, rolling, arg-extreme and exceed
        # queries bypass the plan cache: its plans replay pyas_partial launches)
        if self.resident and self.group is None and self._method is not None and not second and not has_w \
                and not hist and not quant and not co and not tr and not gr and not sp and not ro and not ax \
                and not ex:
            ikey = _index_key(index)
            if ikey is not None:
                cache_key = (ikey, self._norm_axes(), _missing_key(self.missing))
                hit = self._cached_query(cache_key)
                if hit is not _MISS:
                    return hit
        compressor, filters = (None, None) if not ds.filter_pipeline else \
            decode_filters(ds.filter_pipeline, ds.dtype.itemsize, ds.name)
        if sp:
            self._check_spell_index(index)
        if ro:
            self._check_ordered_index(index, self._rolling["along"], "rolling",
                                      "windows follow the selection in increasing order",
                                      "windows follow the selection in order")
        if ax:
            self._check_ordered_index(index, self._argext["along"], self._method,
                                      "positions follow the selection in increasing order",
                                      "positions follow the selection in order")
        indexer = OrthogonalIndexer(index, ds.shape, ds.chunks)
        if self.components and self._method is None:       # active.py:483-485
            raise ValueError("Setting components to True for None statistical method.")
        if self._method is None:
            return self._select(indexer, compressor, filters)
        for i, d in enumerate(indexer.dim_indexers):        # active.py:489-500
            if d.kind == "int":
                raise IndexError("Can't do an active reduction when the index for "
                                 f"axis {i!r} drops the axis.")
        if (second or co) and self._mweights is not None:
            return self._reduce_wmoments(indexer, compressor, filters, self._norm_axes())
        if second:
            return self._reduce_moments(indexer, compressor, filters, self._norm_axes())
        if hist:
            return self._reduce_hist(index, indexer, compressor, filters, self._norm_axes())
        if quant:
            return self._reduce_select(indexer, compressor, filters, self._norm_axes())
        if has_w:
            return self._reduce_weighted(indexer, compressor, filters, self._norm_axes())
        if co:
            return self._reduce_comoments(indexer, compressor, filters, self._norm_axes())
        if tr:
            return self._reduce_trend(indexer, compressor, filters, self._norm_axes())
        if gr:
            return self._reduce_grouped(indexer, compressor, filters, self._norm_axes())
        if sp:
            return self._reduce_spell(indexer, compressor, filters)
        if ro:
            return self._reduce_rolling(indexer, compressor, filters)
        if ax:
            return self._reduce_argext(indexer, compressor, filters)
        if ex:
            return self._reduce_exceed(indexer, compressor, filters, self._norm_axes())
        return self._reduce(indexer, compressor, filters, self._norm_axes(), cache_key)

    def _norm_axes(self):
        """The reduced axes, sorted and non-negative (active.py:505-510)."""
        ndim = self.ds.ndim
        axes = []
        for i in self._axis:
            if not -ndim <= i < ndim:
                raise ValueError(f"Can't do an active reduction for an out-of-range axis: {i!r}")
            axes.append(i % ndim)
        if len(set(axes)) != len(axes):
            raise ValueError("duplicate value in 'axis'")
        return tuple(sorted(axes))

    def _cached_query(self, key):
        """Replay a cached plan of this resident variable (every chunk of the
        query is still in its slot), or _MISS."""
        store = getattr(self.ds, "_pyas_resident", None)
        if store is None or store["device"] != self.device:
            return _MISS
        with _RESIDENT_LOCK:
            entry = store.get("plans", {}).get(key)
            if entry is None or store["released"]:
                return _MISS
            store["users"] += 1
        self._held.stores.append(store)
        return entry.run(self)

    def _remember(self, key, entry):
        store = getattr(self.ds, "_pyas_resident", None)
        if key is None or store is None or entry.plan.batch.data != store["buf"].ptr:
            return
        with _RESIDENT_LOCK:
            plans = store.setdefault("plans", {})
            if len(plans) >= _PLAN_CACHE_CAP:
                plans.pop(next(iter(plans)))
            plans[key] = entry

    # -- host ingest -------------------------------------------------------
    def _ingest(self, coords, compressor, filters):
        """Device buffer + per-chunk offsets of every touched chunk (decoded,
        still byte-shuffled when the shuffle is fused into the kernels).
        ``coords``: chunk coordinate tuples, or an int64 array (n, ndim)."""
        if self.resident:
            got = self._ingest_resident(coords, compressor, filters)
            if got is not None:
                return got
        if isinstance(coords, np.ndarray):
            coords = [tuple(c) for c in coords.tolist()]
        return self._ingest_fresh(coords, compressor, filters)

    def _ingest_resident(self, coords, compressor, filters):
        """Resident mode: the variable's decoded chunks stay in HBM (one slot
        per chunk of the variable's grid, allocated on first use), so a query
        reads from the file only the chunks no earlier query loaded.  None
        when the filter pipeline needs a standalone device pass."""
        ds = self.ds
        shuffles = _shuffle_sizes(filters)
        if shuffles and shuffles[-1] == ds.dtype.itemsize:
            shuffles.pop()
        if any(es > 1 for es in shuffles):
            return None
        nbytes = int(np.prod(ds.chunks)) * ds.dtype.itemsize
        stride = -(-nbytes // _ALIGN) * _ALIGN
        grid = tuple(-(-s // c) for s, c in zip(ds.shape, ds.chunks))
        _check_attached(ds, self.device)
        ctx = get_context(self.device)
        with _RESIDENT_LOCK:
            store = getattr(ds, "_pyas_resident", None)
            _check_attached(ds, self.device)
            if store is None or store["device"] != self.device:
                n_all = int(np.prod(grid))
                store = {"device": self.device, "buf": DeviceBuffer(ctx, max(n_all, 1) * stride),
                         "state": np.zeros(n_all, dtype=np.int8), "users": 0, "released": False}
                ds._pyas_resident = store
            store["users"] += 1
        held = getattr(self._held, "stores", None)
        if held is None:
            held = self._held.stores = []
        held.append(store)
        c = np.asarray(coords, dtype=np.int64).reshape(len(coords), len(grid))
        slots = np.ravel_multi_index(c.T, grid) if len(coords) else np.zeros(0, dtype=np.int64)
        fused = self._fused_shuffle(filters)
        st = ctx.thread_stream()
        while True:
            # claim the empty slots; slots another query is loading are waited for
            with _RESIDENT_LOCK:
                state = store["state"]
                todo = np.nonzero(state[slots] == _EMPTY)[0]
                state[slots[todo]] = _LOADING
            try:
                st = self._load_slots(ctx, store, c[todo], slots[todo], stride, nbytes, compressor,
                                      filters, fused)
            except BaseException:
                with _RESIDENT_CV:
                    store["state"][slots[todo]] = _EMPTY
                    _RESIDENT_CV.notify_all()
                raise
            with _RESIDENT_CV:
                store["state"][slots[todo]] = _LOADED
                _RESIDENT_CV.notify_all()
                while (store["state"][slots] == _LOADING).any():
                    _RESIDENT_CV.wait()
                if (store["state"][slots] == _LOADED).all():
                    break
                # a loader failed: its slots are empty again, claim them
        return ctx, st, store["buf"], slots.astype(np.int64) * stride, 0 if fused in (2, 4, 8) else fused

    def _load_slots(self, ctx, store, coords, slots, stride, nbytes, compressor, filters, fused):
        """Read + decode chunks ``coords`` into resident ``slots``; returns
        the stream, synchronised (other queries read the slots once marked)."""
        st = ctx.thread_stream()
        if not len(slots):
            return st
        todo_coords = [tuple(x) for x in coords.tolist()]
        if fused in (2, 4, 8):
            # the store keeps chunks un-shuffled (one batched pass as they
            # arrive), so every later query takes the unshuffled kernels
            # (dense partial-axis layouts and the in-kernel layer fold)
            _, st, tmp, toffs, _ = self._ingest_fresh(todo_coords, compressor, filters)
            offs = np.concatenate([toffs, slots * stride]).astype(np.int64)
            meta = DeviceBuffer(ctx, offs.nbytes)
            ctx.h2d(meta.ptr, offs, st)
            engine.unshuffle_chunks(ctx, tmp.ptr, meta.ptr, store["buf"].ptr, meta.ptr + 8 * len(slots),
                                    len(slots), nbytes, fused, st)
            ctx.synchronize(st)   # tmp and meta are freed on return
        else:
            _, st, _, _, _ = self._ingest_fresh(todo_coords, compressor, filters,
                                                dst=store["buf"], dst_offsets=slots * stride)
            ctx.synchronize(st)
        return st

    def _ingest_fresh(self, coords, compressor, filters, dst=None, dst_offsets=None):
        """Read + inflate every touched chunk into one device buffer (``dst``
        at ``dst_offsets`` when given)."""
        ds = self.ds
        nbytes = int(np.prod(ds.chunks)) * ds.dtype.itemsize

        zlib_chunks = is_zlib(compressor)
        device_inflate = zlib_chunks and inflate_on_device(len(coords), self._max_threads, self.device_inflate)
        ctx = get_context(self.device)
        st = ctx.thread_stream()
        stride = -(-nbytes // _ALIGN) * _ALIGN
        infos = [ds.chunk_info(c) for c in coords]
        n = len(infos)
        doffs = (np.arange(n, dtype=np.int64) * stride if dst_offsets is None
                 else np.ascontiguousarray(dst_offsets, dtype=np.int64))
        if n == 0:
            buf = dst if dst is not None else DeviceBuffer(ctx, stride)
            return ctx, st, buf, doffs, self._fused_shuffle(filters)
        native_io = ds.reader is None and ds.filename is not None and (zlib_chunks or compressor is None)
        if native_io:
            # f2: native pread ring -> pinned slots -> H2D, no Python per chunk
            foff = np.array([o for o, _ in infos], dtype=np.int64)
            fsize = np.array([z for _, z in infos], dtype=np.int64)
            self.data_read += int(fsize.sum())
            if device_inflate:
                # f2+f3 pipeline: the compressed bytes arrive in groups on a
                # copy stream; each group is inflated on its own stream as soon
                # as its copies land (inflate waves of every group can be
                # resident together: one stream per wave, so concurrency is
                # what buys inflate throughput), while the host reads on
                # compressed streams back to back (the inflater reads any
                # alignment), so file-contiguous chunks stay one H2D copy per
                # staging slot instead of one per chunk
                soffs = np.concatenate([[0], np.cumsum(fsize)[:-1]]).astype(np.int64)
                src = DeviceBuffer(ctx, int(fsize.sum()) + 16)
                buf = dst if dst is not None else DeviceBuffer(ctx, max(n, 1) * stride)
                copy_st = ctx.thread_aux_stream(0)
                ctx.stream_wait(copy_st, st)      # order after prior work on st
                batches = []
                # one launch per ~2048 streams: below that a launch inflates
                # every stream at once (a stream's time is the latency of one
                # serial decoder), so splitting the read/inflate pipeline into
                # launches would only queue them one after another
                groups = _pipeline_groups(fsize, max(1, min(_INFLATE_GROUPS, -(-n // 2048))))
                for g, (lo, hi) in enumerate(groups):
                    read_ranges(ctx, ds.filename, foff[lo:hi], fsize[lo:hi], src.ptr, soffs[lo:hi],
                                copy_st, self._max_threads)
                    inf_st = ctx.thread_aux_stream(1 + g)
                    ctx.stream_wait(inf_st, copy_st)
                    ib = InflateBatch(ctx, soffs[lo:hi], fsize[lo:hi], doffs[lo:hi],
                                      np.full(hi - lo, nbytes, dtype=np.int64))
                    ib.launch(src.ptr, buf.ptr, inf_st)
                    batches.append((lo, ib, inf_st))
                for lo, ib, inf_st in batches:
                    ib.check(inf_st, base=lo)
                    ctx.stream_wait(st, inf_st)
                del src
            elif zlib_chunks:
                # f3 on the host: the reader threads inflate each chunk straight
                # into its pinned staging slot (pyas_read_ranges_zlib), the
                # inflated bytes go H2D
                buf = dst if dst is not None else DeviceBuffer(ctx, max(n, 1) * stride)
                read_ranges_zlib(ctx, ds.filename, foff, fsize, buf.ptr, doffs, nbytes, st, self._max_threads,
                                 reshape=(ds.dtype.itemsize, ds.chunks))
            else:
                bad = np.nonzero(fsize != nbytes)[0]
                if bad.size:   # storage.py:57-62 reshape of a wrongly sized chunk
                    raise ValueError(f"cannot reshape array of size {int(fsize[bad[0]]) // ds.dtype.itemsize} "
                                     f"into shape {ds.chunks}")
                buf = dst if dst is not None else DeviceBuffer(ctx, max(n, 1) * stride)
                read_ranges(ctx, ds.filename, foff, fsize, buf.ptr, doffs, st, self._max_threads)
        else:
            def fetch(info):
                off, size = info
                raw = ds.read(off, size)
                return off, size, (raw if device_inflate else _decompress(raw, compressor))

            with concurrent.futures.ThreadPoolExecutor(max_workers=self._max_threads) as ex:
                blobs = list(ex.map(fetch, infos))
            if device_inflate:
                # f3: one upload of the deflated bytes, one inflate launch into the
                # chunk-major slots the reduce reads (raises like zlib.decompress)
                host, soffs, ssizes = pack_streams([b for _, _, b in blobs])
                self.data_read += int(ssizes.sum())
                src = DeviceBuffer(ctx, host.nbytes)
                ctx.h2d(src.ptr, host, st)
                buf = dst if dst is not None else DeviceBuffer(ctx, max(n, 1) * stride)
                ib = InflateBatch(ctx, soffs, ssizes, doffs, np.full(n, nbytes, dtype=np.int64))
                ib.launch(src.ptr, buf.ptr, st)
                ib.check(st)
                del src
            else:
                host = np.zeros(max(n, 1) * stride, dtype=np.uint8)
                for i, (_, size, b) in enumerate(blobs):
                    a = np.frombuffer(memoryview(b), dtype=np.uint8)
                    if a.size != nbytes:
                        raise ValueError(f"cannot reshape array of size {a.size // ds.dtype.itemsize} "
                                         f"into shape {ds.chunks}")
                    host[i * stride: i * stride + nbytes] = a
                    self.data_read += size
                if dst is None:
                    buf = DeviceBuffer(ctx, host.nbytes)
                    ctx.h2d(buf.ptr, host, st)
                else:
                    buf = dst
                    for i in range(n):
                        ctx.h2d(buf.ptr + int(doffs[i]), host[i * stride: (i + 1) * stride], st)
        shuffles = _shuffle_sizes(filters)
        fused = self._fused_shuffle(filters)
        if shuffles and shuffles[-1] == ds.dtype.itemsize:
            shuffles.pop()
        for es in shuffles:   # non-itemsize shuffles: standalone device pass per chunk
            if es > 1:
                assert dst is None   # resident mode keeps such pipelines out
                tmp = DeviceBuffer(ctx, buf.nbytes)
                for i in range(n):
                    engine.unshuffle(ctx, buf.ptr + i * stride, tmp.ptr + i * stride, nbytes, es, st)
                buf = tmp
        return ctx, st, buf, doffs, fused

    def _fused_shuffle(self, filters):
        """Element size of the shuffle the kernels undo on load (0: none)."""
        shuffles = _shuffle_sizes(filters)
        es = self.ds.dtype.itemsize
        return es if shuffles and shuffles[-1] == es and es > 1 else 0

    @staticmethod
    def _chunk_sel(projs):
        dims = []
        for p in projs:
            s = p.chunk_sel
            if isinstance(s, slice):
                cnt = len(p.out_pos)
                dims.append(selection.DimSel(s.start if cnt else 0, s.step, cnt, False))
            elif isinstance(s, np.ndarray):
                dims.append(selection.DimSel(0, 0, int(s.size), False, s.astype(np.int64)))
            else:
                dims.append(selection.DimSel(int(s), 1, 1, True))
        shape = tuple(d.count for d in dims if not d.dropped)
        kept = tuple(i for i, d in enumerate(dims) if not d.dropped)
        return selection.ChunkSel(dims, shape, kept)

    # -- reductions ---------------------------------------------------------
    def _box_plan(self, indexer):
        """Vectorised plan of an orthogonal selection of slices and index
        arrays: the touched chunks are the C-ordered product of per-dim
        projections (active.py:451-471), so the ABI selection table, index
        pool and chunk coordinates follow from per-dim entries by
        broadcasting, with no per-chunk Python objects.  Returns
        ``(dims, coords, table, pool)`` or None (integer-dropped dims, or
        vector fill/missing values whose masks need per-chunk selections)."""
        if any(d.kind == "int" for d in indexer.dim_indexers):
            return None
        if any(m is not None and np.size(m) != 1 for m in self.missing):
            return None
        dims = [list(d) for d in indexer.dim_indexers]
        nd = len(dims)
        n_coords = [len(p) for p in dims]
        ent, pool_parts, pos = [], [], 0
        for projs in dims:
            e = np.zeros((len(projs), 3), dtype=np.int32)
            for a, p in enumerate(projs):
                sl = p.chunk_sel
                if isinstance(sl, slice):
                    cnt = len(p.out_pos)
                    e[a] = (sl.start if cnt else 0, sl.step, cnt)
                else:
                    e[a] = (pos, 0, sl.size)
                    pool_parts.append(np.asarray(sl, dtype=np.int32))
                    pos += sl.size
            ent.append(e)
        n = int(np.prod(n_coords))
        idx = np.indices(n_coords).reshape(nd, n)
        table = np.zeros((n, _lib.MAX_DIMS, 3), dtype=np.int32)
        table[:, :, 1] = 1
        table[:, :, 2] = 1
        coords = np.zeros((n, nd), dtype=np.int64)
        for d in range(nd):
            table[:, d, :] = ent[d][idx[d]]
            coords[:, d] = np.array([p.chunk_ix for p in dims[d]], dtype=np.int64)[idx[d]]
        pool = np.concatenate(pool_parts) if pool_parts else np.zeros(1, dtype=np.int32)
        return dims, coords, table, pool

    def _reduce(self, indexer, compressor, filters, axes, cache_key=None):
        box = self._box_plan(indexer)
        if box is None:
            if self.group is not None:
                raise NotImplementedError("a distributed Active query needs slices/index lists on every "
                                          "dimension and scalar missing-data attributes")
            return self._reduce_general(indexer, compressor, filters, axes)
        ds = self.ds
        dt = ds.dtype
        dims, coords, table, pool = box
        final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        n_final = int(np.prod(final_shape))
        pdt = engine.partial_dtype(dt)
        n = len(coords)
        lo, hi = 0, n
        if self.group is not None:   # this rank's contiguous chunk range
            import torch.distributed as dist
            from .distributed import shard_ranges
            weights = np.prod(table[:, :ds.ndim, 2].astype(np.int64), axis=1)
            lo, hi = shard_ranges(weights, dist.get_world_size(self.group))[dist.get_rank(self.group)]
        keys = [] if self.group is not None else None
        if hi > lo:
            ctx, st, buf, offsets, fused = self._ingest(coords[lo:hi], compressor, filters)
            sub = table[lo:hi]
            full = _all_full(sub, ds.chunks)   # whole chunks: no table, lean/dense kernels
            plan = ReductionPlan(ctx, dt, ds.chunks, buf.ptr, offsets, shuffle=fused,
                                 sel_table=None if full else sub, index_pool=None if full else pool,
                                 missing=self.missing, round_to_var=True, stream=st)
            cacheable = cache_key is not None and self.resident and self.group is None
            if len(axes) == ds.ndim:
                final = self._total(plan, st, layer_base=lo, n_layers=n, keys=keys)
                if cacheable:
                    self._remember(cache_key, _CachedQuery(plan, final_shape))
            else:
                grid = self._grid_from_dims(dims, axes, final_shape)
                if self.group is None:   # one process: format on the device
                    rec = {} if cacheable else None
                    out = self._grid_partials(ctx, st, plan, grid, axes, final_shape, lo, hi,
                                              formatted=True, rec=rec)
                    if cacheable:
                        self._remember(cache_key, _CachedQuery(plan, final_shape, rec))
                    return out
                final = self._grid_partials(ctx, st, plan, grid, axes, final_shape, lo, hi, keys=keys)
        else:
            final = np.zeros(n_final, dtype=pdt)   # count 0: neutral in every combine
        if self.group is not None:
            if not keys:   # no chunks here, or no zero-sign work: neutral keys
                keys = [np.concatenate([np.zeros(n_final, np.uint64), np.full(n_final, ~np.uint64(0))])]
            lr = n if len(axes) == ds.ndim else \
                zerosign.grid_lr([len(dims[d]) if d in axes else final_shape[d] for d in range(ds.ndim)],
                                 set(axes))
            final = self._exchange(final, keys[0], lr)
        return self._format(final.reshape(final_shape), final_shape)

    # -- var / std ------------------------------------------------------------
    def _query_plan(self, indexer, compressor, filters, axes, pair=None):
        """What a record or counting query launches over: the query's chunks on
        the device and their plan.  A namespace of ``final_shape``, ``n_final``,
        ``axes_mask``, ``coords`` (the chunks' coordinates in launch order),
        ``n``, ``dims`` / ``table`` (a box query) or ``chunk_list`` (anything
        else), and ``empty``; unless the query selects nothing, also ``ctx``,
        ``st``, ``plan`` and ``keep`` (the buffers to hold until the stream is
        synchronised).  ``pair`` (cov / corr): a second Active whose chunks at
        the same coordinates are ingested too, with ``plan_y`` over them and
        the same selections; a vector fill or missing value on either side
        needs per-chunk selections."""
        ds = self.ds
        q = SimpleNamespace(dims=None, table=None, chunk_list=None, axes_mask=_axes_mask(axes))
        q.final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        q.n_final = int(np.prod(q.final_shape))
        missing_y = get_missing_attributes(pair.ds.attrs) if pair is not None else ()
        box = None if any(m is not None and np.size(m) != 1 for m in missing_y) else self._box_plan(indexer)
        if box is not None:
            q.dims, q.coords, q.table, pool = box
        else:
            q.chunk_list = list(indexer)
            q.coords = [c for c, _ in q.chunk_list]
        q.n = len(q.coords)
        q.empty = q.n == 0 or q.n_final == 0
        if q.empty:
            return q
        q.ctx, q.st, buf, offsets, fused = self._ingest(q.coords, compressor, filters)
        q.keep = [buf]
        if pair is not None and pair is not self:
            _, yst, ybuf, yoffsets, yfused = self._ingest_other(pair, q.coords)
            if yst != q.st:    # (one stream per thread and device: both ingests share it)
                q.ctx.stream_wait(q.st, yst)
            q.keep.append(ybuf)
        elif pair is not None:
            ybuf, yoffsets, yfused = buf, offsets, fused
        if box is not None:
            full = _all_full(q.table, ds.chunks)   # whole chunks: no table
            sel = dict(sel_table=None if full else q.table, index_pool=None if full else pool)
        else:
            sel = dict(selections=[self._chunk_sel(projs) for _, projs in q.chunk_list])
        q.plan = ReductionPlan(q.ctx, ds.dtype, ds.chunks, buf.ptr, offsets, shuffle=fused, missing=self.missing,
                               stream=q.st, **sel)
        if pair is not None:
            q.plan_y = ReductionPlan(q.ctx, pair.ds.dtype, pair.ds.chunks, ybuf.ptr, yoffsets, shuffle=yfused,
                                     missing=missing_y, stream=q.st, **sel)
        return q

    def _reduce_records(self, q, axes, nb, launch, combine_segments, combine_grid, fin=None):
        """The per-chunk pass of a record query (``launch(out_offsets_ptr,
        out_ptr)``, records of ``nb`` bytes) and the merge of its records, in
        the order the sums are combined in: a full reduction in chunk order
        (:func:`_fold_levels`), a box query over the chunk layers of each
        output (``combine_grid``), anything else over host-built segments
        (``combine_segments``).  Returns the device buffer of the ``n_final``
        combined records and the buffers to hold until the stream is
        synchronised."""
        ctx, st, n = q.ctx, q.st, q.n
        ndim = self.ds.ndim
        if fin is None:
            fin = DeviceBuffer(ctx, q.n_final * nb)
        if len(axes) == ndim:
            # one allocation: every level's records, then every level's segment bounds
            levels, n_rec = _fold_levels(n)
            segs = np.concatenate([seg for _, seg in levels])
            work = DeviceBuffer(ctx, n_rec * nb + segs.nbytes)
            cur, sptr = work.ptr, work.ptr + n_rec * nb
            ctx.h2d(sptr, segs, st)
            launch(None, cur)
            nxt = cur + n * nb
            for n_seg, seg in levels:
                dst = fin.ptr if n_seg == 1 else nxt
                combine_segments(ctx, cur, None, sptr, n_seg, dst, st)
                cur, nxt, sptr = dst, dst + n_seg * nb, sptr + seg.nbytes
            return fin, [work]
        if q.dims is not None:
            out_off, tables = self._grid_from_dims(q.dims, axes, q.final_shape)
            obuf = DeviceBuffer(ctx, out_off.nbytes)
            ctx.h2d(obuf.ptr, out_off, st)
            tbuf = DeviceBuffer(ctx, max(tables["blob"].nbytes, 16))
            ctx.h2d(tbuf.ptr, tables["blob"], st)
            g = _grid_struct(ndim, axes, q.final_shape, tables, tbuf.ptr, obuf.ptr)
            parts = DeviceBuffer(ctx, max(int(tables["n_parts"]), 1) * nb)
            launch(obuf.ptr, parts.ptr)
            combine_grid(ctx, parts.ptr, g, fin.ptr, st)
            return fin, [obuf, tbuf, parts]
        out_off, order, seg = _segment_meta((projs for _, projs in q.chunk_list), axes, q.final_shape)
        meta = np.concatenate([out_off[:-1], order, seg])
        mbuf = DeviceBuffer(ctx, meta.nbytes)
        ctx.h2d(mbuf.ptr, meta, st)
        parts = DeviceBuffer(ctx, max(int(out_off[-1]), 1) * nb)
        launch(mbuf.ptr, parts.ptr)
        combine_segments(ctx, parts.ptr, mbuf.ptr + 8 * n, mbuf.ptr + 8 * (n + order.size), q.n_final, fin.ptr, st)
        return fin, [mbuf, parts]

    def _records_back(self, q, fin, keep, dtype):
        """The combined records of a record query on the host; ``keep`` (the
        buffers its launches use) lives until the stream is synchronised."""
        final = np.zeros(q.n_final, dtype=dtype)
        q.ctx.d2h(final, fin.ptr, q.st)
        q.ctx.synchronize(q.st)
        return final.reshape(q.final_shape)

    def _reduce_moments(self, indexer, compressor, filters, axes):
        """var / std: per-chunk count / mean / m2 records (pyas_moments_axes)
        merged with Chan's formula in the orders of :meth:`_reduce_records`."""
        q = self._query_plan(indexer, compressor, filters, axes)
        if q.empty:
            return self._format_moments(np.zeros(q.final_shape, dtype=engine.moments_dtype))

        def launch(off_ptr, out_ptr):
            engine.moments_axes(q.ctx, q.plan.batch, q.plan.mask_up.struct, q.axes_mask, off_ptr, out_ptr, q.st)
        fin, keep = self._reduce_records(q, axes, _lib.MOMENTS_NBYTES, launch, engine.moments_combine_segments,
                                         engine.moments_combine_grid)
        return self._format_moments(self._records_back(q, fin, keep, engine.moments_dtype))

    # -- cov / corr -----------------------------------------------------------
    def _ingest_other(self, other, coords):
        """``other``'s chunks ``coords`` through its own ingest (its filter
        pipeline, its resident store); the stores it holds join this query's,
        so ``__getitem__`` releases both sides together."""
        yds = other.ds
        compressor, filters = (None, None) if not yds.filter_pipeline else \
            decode_filters(yds.filter_pipeline, yds.dtype.itemsize, yds.name)
        prev = getattr(other._held, "stores", None)
        other._held.stores = self._held.stores
        other.data_read = 0
        try:
            got = other._ingest(coords, compressor, filters)
        finally:
            other._held.stores = prev
        self.data_read += other.data_read
        return got

    def _reduce_comoments(self, indexer, compressor, filters, axes):
        """cov / corr: per-chunk count / means / m2s / cxy records of the two
        variables' pairs (pyas_comoments_axes: one plan per side, over the same
        chunk list and selections) merged in the orders of
        :meth:`_reduce_records`."""
        q = self._query_plan(indexer, compressor, filters, axes, pair=self._co)
        if q.empty:
            return self._format_comoments(np.zeros(q.final_shape, dtype=engine.comoments_dtype))

        def launch(off_ptr, out_ptr):
            engine.comoments_axes(q.ctx, q.plan.batch, q.plan.mask_up.struct, q.plan_y.batch, q.plan_y.mask_up.struct,
                                  q.axes_mask, off_ptr, out_ptr, q.st)
        fin, keep = self._reduce_records(q, axes, _lib.COMOMENTS_NBYTES, launch, engine.comoments_combine_segments,
                                         engine.comoments_combine_grid)
        return self._format_comoments(self._records_back(q, fin, keep, engine.comoments_dtype))

    # -- trend -------------------------------------------------------------------
    def _coord_tables(self, coords):
        """pyas_coord of this query for the chunks at ``coords``: the coordinate
        vector zero-padded to whole chunks (so that every entry of an edge chunk
        is readable) and each chunk's origin in it (:meth:`_weight_tables` for
        one dim)."""
        ds = self.ds
        d = self._trend["along"]
        coords = np.asarray(coords, dtype=np.int64).reshape(-1, ds.ndim)
        padded = np.zeros(-(-ds.shape[d] // ds.chunks[d]) * ds.chunks[d], dtype=np.float64)
        padded[:ds.shape[d]] = self._trend["coord"]
        if padded.size >= 2 ** 31:
            raise NotImplementedError("coordinate vectors of 2^31 entries or more")
        return padded, (coords[:, d] * ds.chunks[d]).astype(np.int32)

    def _reduce_trend(self, indexer, compressor, filters, axes):
        """trend: co-moment records of the data against the coordinate.  A
        unit-step box query whose reduced axes are a leading prefix of the dims
        takes the dense column kernel (pyas_trend_cols: one finished record per
        output, the chunk layers folded in the kernel); anything else
        per-chunk records (pyas_trend_axes) merged in the orders of
        :meth:`_reduce_records`.  The slope and its mask are computed on the
        device (pyas_trend_finalize) unless ``components`` is set."""
        ds = self.ds
        along = self._trend["along"]
        self._trend_path = None
        q = self._query_plan(indexer, compressor, filters, axes)
        final_shape, n_final = q.final_shape, q.n_final
        if q.empty:
            return self._format_trend(np.zeros(final_shape, dtype=engine.comoments_dtype))
        ctx, st, plan = q.ctx, q.st, q.plan
        fin = DeviceBuffer(ctx, n_final * _lib.COMOMENTS_NBYTES)
        cpool, corigin = self._coord_tables(q.coords)
        cbuf = DeviceBuffer(ctx, cpool.nbytes + corigin.nbytes)
        ctx.h2d(cbuf.ptr, cpool, st)
        ctx.h2d(cbuf.ptr + cpool.nbytes, corigin, st)

        def launch(off_ptr, out_ptr):
            engine.trend_axes(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, along,
                              q.axes_mask, off_ptr, out_ptr, st)
        # the dense path: every dim one unit-step range, reduced axes 0 .. P-1, a kept dim behind them
        dense = q.dims is not None and len(axes) < ds.ndim and axes == tuple(range(len(axes))) \
            and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done = False
        if dense:
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.trend_cols(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, along, g,
                                     fin.ptr, st)
        keep = []
        if not done:
            fin, keep = self._reduce_records(q, axes, _lib.COMOMENTS_NBYTES, launch,
                                             engine.comoments_combine_segments, engine.comoments_combine_grid, fin=fin)
        self._trend_path = "cols" if done else "walk"
        if self._components:
            # the records, and the slope and intercept computed on the device
            vbuf = DeviceBuffer(ctx, n_final * 17)
            sl, ic = np.empty(n_final, dtype=np.float64), np.empty(n_final, dtype=np.float64)
            engine.trend_finalize(ctx, fin.ptr, n_final, _lib.TREND_SLOPE, vbuf.ptr, vbuf.ptr + 16 * n_final, st)
            engine.trend_finalize(ctx, fin.ptr, n_final, _lib.TREND_INTERCEPT, vbuf.ptr + 8 * n_final,
                                  vbuf.ptr + 16 * n_final, st)
            final = np.zeros(n_final, dtype=engine.comoments_dtype)
            ctx.d2h(final, fin.ptr, st)
            ctx.d2h(sl, vbuf.ptr, st)
            ctx.d2h(ic, vbuf.ptr + 8 * n_final, st)
            ctx.synchronize(st)
            del keep
            return self._format_trend(final.reshape(final_shape), sl.reshape(final_shape), ic.reshape(final_shape))
        # the slope and its mask on the device: 9 bytes per output come back
        vbuf = DeviceBuffer(ctx, n_final * 9)
        engine.trend_finalize(ctx, fin.ptr, n_final, _lib.TREND_SLOPE, vbuf.ptr, vbuf.ptr + 8 * n_final, st)
        val = np.empty(n_final, dtype=np.float64)
        msk = np.empty(n_final, dtype=np.uint8)
        ctx.d2h(val, vbuf.ptr, st)
        ctx.d2h(msk, vbuf.ptr + 8 * n_final, st)
        ctx.synchronize(st)
        del keep
        return np.ma.MaskedArray(val.reshape(final_shape), mask=msk.reshape(final_shape).astype(bool))

    def _format_trend(self, parts, slope=None, intercept=None):
        """The float64 result of a trend query from its combined records on
        the host (trend.slope), or its components (``slope`` / ``intercept``:
        their values as pyas_trend_finalize computed them, else computed
        here)."""
        if self._components:
            empty = parts["count"] == 0
            out = {name: np.ma.MaskedArray(np.ascontiguousarray(parts[name]), mask=empty)
                   for name in ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")}
            out["n"] = np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                         mask=np.zeros(parts.shape, dtype=bool))
            out["slope"] = trend.slope(parts) if slope is None else np.ma.MaskedArray(slope, mask=empty)
            out["intercept"] = trend.intercept(parts) if intercept is None else \
                np.ma.MaskedArray(intercept, mask=empty)
            return out
        return trend.slope(parts)

    # -- spell -------------------------------------------------------------------
    def _check_spell_index(self, index):
        """The index along the spell dimension keeps the elements in order: a
        slice of step >= 1, a strictly increasing index list or a boolean
        mask.  ValueError otherwise (what no statistic accepts is left to the
        planner's own errors)."""
        self._check_ordered_index(index, self._spell["along"], "spell",
                                  "runs follow the selection in increasing order",
                                  "runs follow the selection in order")

    def _check_ordered_index(self, index, d, who, why_step, why_list):
        """The order check of :meth:`_check_spell_index` for the statistic
        ``who`` along dimension ``d`` (``why_*``: the reason its messages
        give)."""
        s = _normalize(index, self.ds.ndim)[d]
        if isinstance(s, slice):
            if isinstance(s.step, (int, np.integer)) and s.step < 1:
                raise ValueError(f"{who}: the slice along dimension {d} has step {s.step}; {why_step}, so the step "
                                 "must be >= 1")
            return
        if isinstance(s, (list, np.ndarray)) and np.ndim(s) > 0:
            a = np.asarray(s)
            if a.ndim == 1 and a.dtype.kind in "iu":
                a = np.where(a < 0, a.astype(np.int64) + self.ds.shape[d], a.astype(np.int64))
                if a.size > 1 and not bool(np.all(np.diff(a) > 0)):
                    raise ValueError(f"{who}: the index list along dimension {d} must be strictly increasing "
                                     f"(no repeats): {why_list}")
            return
        raise ValueError(f"{who}: the index along dimension {d} must be a slice, an increasing index list or a "
                         f"boolean mask. Got {s!r}")

    def _reduce_spell(self, indexer, compressor, filters):
        """spell: records of the runs along the one reduced axis.  A unit-step
        box query with ``along == 0`` and a dim behind it takes the dense
        column kernel (pyas_spell_cols: one finished record per output, the
        chunk layers walked in the kernel); anything else per-chunk records
        (pyas_spell_axes) merged in the orders of :meth:`_reduce_records`,
        each of which folds the chunks of an output in increasing chunk order
        along the axis.  The statistic and its mask are computed on the device
        (pyas_spell_finalize) unless ``components`` is set."""
        ds = self.ds
        sp = self._spell
        along, axes = sp["along"], (sp["along"],)
        self._spell_path = None
        if indexer.dim_indexers[along].nitems >= 2 ** 31:
            raise NotImplementedError(f"spell: {indexer.dim_indexers[along].nitems} selected positions along "
                                      f"dimension {along}; the record counts in int32 (fewer than 2^31)")
        q = self._query_plan(indexer, compressor, filters, axes)
        final_shape, n_final = q.final_shape, q.n_final
        if q.empty:
            return self._format_spell(np.zeros(final_shape, dtype=engine.spell_dtype))
        ctx, st, plan = q.ctx, q.st, q.plan
        rule = (along, sp["op"], sp["threshold"], sp["min_length"])
        fin = DeviceBuffer(ctx, n_final * _lib.SPELL_NBYTES)

        def launch(off_ptr, out_ptr):
            engine.spell_axes(ctx, plan.batch, plan.mask_up.struct, *rule, off_ptr, out_ptr, st)
        # the dense path: every dim one unit-step range, axis 0 reduced, a kept dim behind it
        dense = q.dims is not None and axes == (0,) and ds.ndim > 1 and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done = False
        if dense:
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.spell_cols(ctx, plan.batch, plan.mask_up.struct, *rule, g, fin.ptr, st)
        keep = []
        if not done:
            fin, keep = self._reduce_records(q, axes, _lib.SPELL_NBYTES, launch, engine.spell_combine_segments,
                                             engine.spell_combine_grid, fin=fin)
        self._spell_path = "cols" if done else "walk"
        if self._components:
            final = self._records_back(q, fin, keep, engine.spell_dtype)
            del keep
            return self._format_spell(final)
        # the statistic and its mask on the device: 5 bytes per output come back
        vbuf = DeviceBuffer(ctx, n_final * 5)
        engine.spell_finalize(ctx, fin.ptr, n_final, sp["stat"], vbuf.ptr, vbuf.ptr + 4 * n_final, st)
        val = np.empty(n_final, dtype=np.int32)
        msk = np.empty(n_final, dtype=np.uint8)
        ctx.d2h(val, vbuf.ptr, st)
        ctx.d2h(msk, vbuf.ptr + 4 * n_final, st)
        ctx.synchronize(st)
        del keep
        return np.ma.MaskedArray(val.reshape(final_shape).astype(np.int64), mask=msk.reshape(final_shape).astype(bool))

    def _format_spell(self, parts):
        """The int64 result of a spell query from its combined records on the
        host (spell.finalize), or its components: the record's fields, and the
        three statistics finalized."""
        if self._components:
            out = {name: np.ma.MaskedArray(np.ascontiguousarray(parts[name]).astype(np.int64),
                                           mask=np.zeros(parts.shape, dtype=bool)) for name in spell.FIELDS}
            out["longest"] = spell.finalize(parts, "longest")
            out["days_total"] = spell.finalize(parts, "days")
            out["events_total"] = spell.finalize(parts, "events")
            return out
        return spell.finalize(parts, self._spell["stat"])

    # -- rolling -----------------------------------------------------------------
    def _reduce_rolling(self, indexer, compressor, filters):
        """rolling: records of the window sums along the one reduced axis.  A
        unit-step box query with ``along == 0`` and a dim behind it takes the
        dense column kernel (pyas_roll_cols: one finished record per output,
        the chunk layers walked in the kernel); anything else per-chunk
        records (pyas_roll_axes) merged in the orders of
        :meth:`_reduce_records`, each of which folds the chunks of an output
        in increasing chunk order along the axis.  The value and its mask are
        computed on the device (pyas_roll_finalize) unless ``components`` is
        set."""
        ds = self.ds
        ro = self._rolling
        along, axes = ro["along"], (ro["along"],)
        self._rolling_path = None
        if indexer.dim_indexers[along].nitems >= 2 ** 31:
            raise NotImplementedError(f"rolling: {indexer.dim_indexers[along].nitems} selected positions along "
                                      f"dimension {along}; the record counts in int32 (fewer than 2^31)")
        q = self._query_plan(indexer, compressor, filters, axes)
        final_shape, n_final = q.final_shape, q.n_final
        if q.empty:
            return self._format_rolling(np.zeros(final_shape, dtype=engine.roll_dtype))
        ctx, st, plan = q.ctx, q.st, q.plan
        rule = (along, ro["window"], ro["which"])
        fin = DeviceBuffer(ctx, n_final * _lib.ROLL_NBYTES)

        def launch(off_ptr, out_ptr):
            engine.roll_axes(ctx, plan.batch, plan.mask_up.struct, *rule, off_ptr, out_ptr, st)
        # the dense path: every dim one unit-step range, axis 0 reduced, a kept dim behind it
        dense = q.dims is not None and axes == (0,) and ds.ndim > 1 and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done = False
        if dense:
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.roll_cols(ctx, plan.batch, plan.mask_up.struct, *rule, g, fin.ptr, st)
        keep = []
        if not done:
            fin, keep = self._reduce_records(q, axes, _lib.ROLL_NBYTES, launch, engine.roll_combine_segments,
                                             engine.roll_combine_grid, fin=fin)
        self._rolling_path = "cols" if done else "walk"
        if self._components:
            final = self._records_back(q, fin, keep, engine.roll_dtype)
            del keep
            return self._format_rolling(final)
        # the value and its mask on the device: 9 bytes per output come back
        vbuf = DeviceBuffer(ctx, n_final * 9)
        engine.roll_finalize(ctx, fin.ptr, n_final, ro["stat"], vbuf.ptr, vbuf.ptr + 8 * n_final, st)
        val = np.empty(n_final, dtype=np.float64)
        msk = np.empty(n_final, dtype=np.uint8)
        ctx.d2h(val, vbuf.ptr, st)
        ctx.d2h(msk, vbuf.ptr + 8 * n_final, st)
        ctx.synchronize(st)
        del keep
        return np.ma.MaskedArray(val.reshape(final_shape), mask=msk.reshape(final_shape).astype(bool))

    def _format_rolling(self, parts):
        """The float64 result of a rolling query from its combined records on
        the host (rolling.finalize), or its components: the finalized value,
        the winning window and the counts, and the record's fields."""
        value = rolling.finalize(parts, self._rolling["stat"])
        if not self._components:
            return value
        bad = np.ma.getmaskarray(value)
        never = np.zeros(parts.shape, dtype=bool)
        out = {name: np.ascontiguousarray(parts[name]) for name in rolling.FIELDS}
        out["value"] = value
        out["sum"] = rolling.finalize(parts, "sum")
        out["position"] = np.ma.MaskedArray(parts["position"].astype(np.int64), mask=bad)
        for name in ("n_windows", "n", "len"):
            out[name] = np.ma.MaskedArray(parts[name].astype(np.int64), mask=never)
        return out

    # -- argmax / argmin ---------------------------------------------------------
    def _reduce_argext(self, indexer, compressor, filters):
        """argmax / argmin: records of the winning element along the one
        reduced axis.  A unit-step box query with ``along == 0`` and a dim
        behind it takes the dense column kernel (pyas_argext_cols: one
        finished record per output, the chunk layers walked in the kernel);
        anything else per-chunk records (pyas_argext_axes) merged in the
        orders of :meth:`_reduce_records`.  The index and its mask come back
        from the device (pyas_argext_finalize) unless ``components`` is set;
        the host turns the global index into the position in the selection."""
        ds = self.ds
        ae = self._argext
        along, which, axes = ae["along"], ae["which"], (ae["along"],)
        self._argext_path = None
        dim = indexer.dim_indexers[along]
        if dim.nitems >= 2 ** 31 or dim.nchunks * ds.chunks[along] >= 2 ** 31:
            raise NotImplementedError(f"{ae['name']}: {dim.nitems} selected positions of {ds.shape[along]} along "
                                      f"dimension {along}; the record holds the index in int32 (fewer than 2^31)")
        q = self._query_plan(indexer, compressor, filters, axes)
        final_shape, n_final = q.final_shape, q.n_final
        if q.empty:
            return self._format_argext(np.zeros(final_shape, dtype=engine.argext_dtype), dim)
        ctx, st, plan = q.ctx, q.st, q.plan
        # origin[c]: the global index of chunk c's local index 0 along the axis
        coords = np.asarray(q.coords, dtype=np.int64).reshape(-1, ds.ndim)
        origin = (coords[:, along] * ds.chunks[along]).astype(np.int32)
        obuf = DeviceBuffer(ctx, origin.nbytes)
        ctx.h2d(obuf.ptr, origin, st)
        fin = DeviceBuffer(ctx, n_final * _lib.ARGEXT_NBYTES)

        def launch(off_ptr, out_ptr):
            engine.argext_axes(ctx, plan.batch, plan.mask_up.struct, along, which, obuf.ptr, off_ptr, out_ptr, st)

        def combine_segments(ctx, *args):
            engine.argext_combine_segments(ctx, ds.dtype, which, *args)

        def combine_grid(ctx, *args):
            engine.argext_combine_grid(ctx, ds.dtype, which, *args)
        # the dense path: every dim one unit-step range, axis 0 reduced, a kept dim behind it
        dense = q.dims is not None and axes == (0,) and ds.ndim > 1 and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done = False
        if dense:
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.argext_cols(ctx, plan.batch, plan.mask_up.struct, along, which, obuf.ptr, g, fin.ptr, st)
        keep = []
        if not done:
            fin, keep = self._reduce_records(q, axes, _lib.ARGEXT_NBYTES, launch, combine_segments, combine_grid,
                                             fin=fin)
        self._argext_path = "cols" if done else "walk"
        if self._components:
            final = self._records_back(q, fin, keep, engine.argext_dtype)
            del keep, obuf
            return self._format_argext(final, dim)
        # the index and its mask on the device: 5 bytes per output come back
        vbuf = DeviceBuffer(ctx, n_final * 5)
        engine.argext_finalize(ctx, fin.ptr, n_final, vbuf.ptr, vbuf.ptr + 4 * n_final, st)
        val = np.empty(n_final, dtype=np.int32)
        msk = np.empty(n_final, dtype=np.uint8)
        ctx.d2h(val, vbuf.ptr, st)
        ctx.d2h(msk, vbuf.ptr + 4 * n_final, st)
        ctx.synchronize(st)
        del keep, obuf
        bad = msk.reshape(final_shape).astype(bool)
        return np.ma.MaskedArray(_selection_position(val.reshape(final_shape).astype(np.int64), bad, dim), mask=bad)

    def _format_argext(self, parts, dim):
        """The int64 result of an argmax / argmin query from its combined
        records on the host (``dim``: the indexer of the axis), or its
        components."""
        index = argext.finalize(parts)
        bad = np.ma.getmaskarray(index)
        pos = np.ma.MaskedArray(_selection_position(index.data.copy(), bad, dim), mask=bad)
        if self._components:
            return {"position": pos, "index": index,
                    "value": np.ma.MaskedArray(argext.values(parts, self.ds.dtype), mask=bad),
                    "n": np.ma.MaskedArray(parts["n"].astype(np.int64), mask=np.zeros(parts.shape, dtype=bool))}
        return pos

    # -- exceed ------------------------------------------------------------------
    def _exceed_field_tables(self, q, axes):
        """pyas_exceed_field of this query for the chunks at ``q.coords``: the
        field's element strides (0 on reduced dims) and each chunk's origin in
        it (two NumPy expressions: nothing loops per chunk or per output)."""
        ds = self.ds
        stride = np.zeros(ds.ndim, dtype=np.int64)
        step = 1
        for d in range(ds.ndim - 1, -1, -1):
            if d not in axes:
                stride[d] = step
                step *= ds.shape[d]
        coords = np.asarray(q.coords, dtype=np.int64).reshape(-1, ds.ndim)
        origin = (coords * np.asarray(ds.chunks, dtype=np.int64)) @ stride
        return stride, np.ascontiguousarray(origin, dtype=np.int64)

    @staticmethod
    def _exceed_thr_masked(indexer, field, axes):
        """The field's mask at the selection, in the final outputs' order
        (uint8, flat), or None when no entry is masked."""
        if field.mask is None:
            return None
        picks = []
        for d, dim in enumerate(indexer.dim_indexers):
            if d in axes:
                picks.append(np.zeros(1, dtype=np.int64))
            elif dim.kind == "slice":
                picks.append(np.arange(dim.start, dim.stop, dim.step, dtype=np.int64))
            else:
                picks.append(dim.sel)
        return np.ascontiguousarray(field.mask[np.ix_(*picks)], dtype=np.uint8).reshape(-1)

    def _reduce_exceed(self, indexer, compressor, filters, axes):
        """exceed: records of the counts and sums past the threshold.  A
        unit-step box query whose reduced axes are a leading prefix of the dims
        takes the dense column kernel (pyas_exceed_cols: one finished record
        per output, the chunk layers walked in the kernel); anything else
        per-chunk records (pyas_exceed_axes) merged in the orders of
        :meth:`_reduce_records`.  A threshold field is uploaded as it is, with
        one origin per chunk (the kernels index it by global index).  The
        statistic and its mask are computed on the device
        (pyas_exceed_finalize) unless ``components`` is set."""
        ds = self.ds
        ex = self._exceed
        field, stat = ex["field"], ex["stat"]
        self._exceed_path = None
        if axes != ex["axes"]:
            raise ValueError(f"exceed: the reduced axes changed from {ex['axes']} to {axes} after the threshold was "
                             "checked against them")
        q = self._query_plan(indexer, compressor, filters, axes)
        final_shape, n_final = q.final_shape, q.n_final
        thr_masked = np.ones(n_final, dtype=np.uint8) if field.all_masked else \
            self._exceed_thr_masked(indexer, field, axes)
        if q.empty:
            return self._format_exceed(np.zeros(final_shape, dtype=engine.exceed_dtype), thr_masked)
        ctx, st, plan = q.ctx, q.st, q.plan
        fin = DeviceBuffer(ctx, n_final * _lib.EXCEED_NBYTES)
        fbuf = None
        if field.values is not None:
            stride, origin = self._exceed_field_tables(q, axes)
            fbuf = DeviceBuffer(ctx, field.values.nbytes + origin.nbytes)
            ctx.h2d(fbuf.ptr, field.values, st)
            ctx.h2d(fbuf.ptr + field.values.nbytes, origin, st)
            rule = engine.exceed_rule(ex["op"], 0.0, (fbuf.ptr, fbuf.ptr + field.values.nbytes, stride))
        else:
            rule = engine.exceed_rule(ex["op"], field.scalar)

        def launch(off_ptr, out_ptr):
            engine.exceed_axes(ctx, plan.batch, plan.mask_up.struct, rule, q.axes_mask, off_ptr, out_ptr, st)
        # the dense path: every dim one unit-step range, reduced axes 0 .. P-1, a kept dim behind them
        dense = q.dims is not None and len(axes) < ds.ndim and axes == tuple(range(len(axes))) \
            and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done = False
        if dense:
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.exceed_cols(ctx, plan.batch, plan.mask_up.struct, rule, g, fin.ptr, st)
        keep = []
        if not done:
            fin, keep = self._reduce_records(q, axes, _lib.EXCEED_NBYTES, launch, engine.exceed_combine_segments,
                                             engine.exceed_combine_grid, fin=fin)
        self._exceed_path = "cols" if done else "walk"
        if self._components:
            final = self._records_back(q, fin, keep, engine.exceed_dtype)
            del keep, fbuf
            return self._format_exceed(final, thr_masked)
        # the statistic and its mask on the device: 9 bytes per output come back
        tm_bytes = n_final if thr_masked is not None else 0
        vbuf = DeviceBuffer(ctx, n_final * 9 + tm_bytes)
        tm_ptr = None
        if thr_masked is not None:
            tm_ptr = vbuf.ptr + 9 * n_final
            ctx.h2d(tm_ptr, thr_masked, st)
        engine.exceed_finalize(ctx, fin.ptr, n_final, stat, tm_ptr, vbuf.ptr, vbuf.ptr + 8 * n_final, st)
        val = np.empty(n_final, dtype=np.int64 if stat == "count" else np.float64)
        msk = np.empty(n_final, dtype=np.uint8)
        ctx.d2h(val, vbuf.ptr, st)
        ctx.d2h(msk, vbuf.ptr + 8 * n_final, st)
        ctx.synchronize(st)
        del keep, fbuf
        return np.ma.MaskedArray(val.reshape(final_shape), mask=msk.reshape(final_shape).astype(bool))

    def _format_exceed(self, parts, thr_masked):
        """The result of an exceed query from its combined records on the host
        (exceed.finalize), or its components; ``thr_masked``: the flat bytes of
        :meth:`_exceed_thr_masked` or None."""
        tm = None if thr_masked is None else thr_masked.reshape(parts.shape).astype(bool)
        if self._components:
            if tm is not None and tm.any():   # (a one-entry masked field ran as a scalar)
                parts = parts.copy()
                for name in ("n_true", "sum", "excess"):
                    parts[name][tm] = 0
            return {name: np.ma.MaskedArray(np.ascontiguousarray(parts[name]), mask=np.zeros(parts.shape, dtype=bool))
                    for name in exceed.FIELDS}
        return exceed.finalize(parts, self._exceed["stat"], tm)

    # -- grouped -----------------------------------------------------------------
    def _reduce_grouped(self, indexer, compressor, filters, axes):
        """grouped: one moments record per (output, group).  A unit-step box
        query whose reduced axes are a leading prefix of the dims takes the
        dense column kernel over the sorted row list (pyas_group_cols: one
        finished record per output and group, nothing merged); anything else
        per-chunk, per-local-group records (pyas_group_axes) merged over
        host-built segments in chunk order (pyas_moments_combine_segments)."""
        ds = self.ds
        gs = self._grouped
        along, labels, n_g = gs["along"], gs["labels"], gs["n_groups"]
        # min / max / sum: the same two walks over pyas_partial records (32 bytes as well), merged by
        # pyas_combine_segments and formatted on the device
        part = gs["stat"] in grouped.PARTIAL_STATS
        rdt = engine.partial_dtype(ds.dtype) if part else engine.moments_dtype
        self._grouped_path = None
        final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        rshape = tuple(n_g if i == along else n for i, n in enumerate(final_shape))
        n_rec = int(np.prod(rshape))
        if n_rec * _lib.MOMENTS_NBYTES > histogram.TABLE_CAP_BYTES:
            raise ValueError(f"grouped: {int(np.prod(final_shape))} outputs of {n_g} groups need "
                             f"{n_rec * _lib.MOMENTS_NBYTES} bytes of records, above the cap of "
                             f"{histogram.TABLE_CAP_BYTES} bytes")
        if n_rec == 0:
            return self._format_grouped(np.zeros(rshape, dtype=rdt))
        q = self._query_plan(indexer, compressor, filters, axes)
        if q.empty:
            return self._format_grouped(np.zeros(rshape, dtype=rdt))
        ctx, st, plan = q.ctx, q.st, q.plan
        nb = _lib.MOMENTS_NBYTES
        fin = DeviceBuffer(ctx, n_rec * nb)
        # the dense path: every dim one unit-step range, reduced axes 0 .. P-1, a kept dim behind them
        dense = q.dims is not None and len(axes) < ds.ndim and axes == tuple(range(len(axes))) \
            and bool(np.all(q.table[:, :ds.ndim, 1] == 1))
        done, keep = False, []
        if dense:
            rows = grouped.row_list(q.dims[:len(axes)], ds.chunks, labels, along, n_g)
            blob = np.concatenate([rows.layer, rows.offset, rows.label, np.zeros(1, dtype=np.int32)])
            rbuf = DeviceBuffer(ctx, blob.nbytes)
            ctx.h2d(rbuf.ptr, blob, st)
            g = _grid_struct(ds.ndim, axes, final_shape, {"n_coords": [len(p) for p in q.dims]}, None, None)
            done = engine.group_cols(ctx, plan.batch, plan.mask_up.struct, rbuf.ptr, rbuf.ptr + 4 * rows.n_rows,
                                     rbuf.ptr + 8 * rows.n_rows, rows.n_rows, n_g, g, fin.ptr, st, partial=part)
            keep = [rbuf, blob]
        if not done:
            projs = itertools.product(*q.dims) if q.dims is not None else (p for _, p in q.chunk_list)
            cl = grouped.chunk_lists(projs, ds.chunks, labels, along, axes, final_shape, n_g)
            n = q.n
            meta = np.concatenate([cl.out_off[:-1], cl.order, cl.seg])
            lists = np.concatenate([cl.chunk_start, cl.ptr, cl.pos, np.zeros(1, dtype=np.int32)])
            mbuf = DeviceBuffer(ctx, meta.nbytes)
            ctx.h2d(mbuf.ptr, meta, st)
            lbuf = DeviceBuffer(ctx, lists.nbytes)
            ctx.h2d(lbuf.ptr, lists, st)
            parts = DeviceBuffer(ctx, max(int(cl.out_off[-1]), 1) * nb)
            engine.group_axes(ctx, plan.batch, plan.mask_up.struct, lbuf.ptr, lbuf.ptr + 4 * cl.chunk_start.size,
                              lbuf.ptr + 4 * (cl.chunk_start.size + cl.ptr.size), along, q.axes_mask, mbuf.ptr,
                              parts.ptr, st, partial=part)
            if part:   # (no rounding to the variable dtype between chunks: the f64 sum is rounded once, at the end)
                engine.combine_segments(ctx, ds.dtype, parts.ptr, mbuf.ptr + 8 * n,
                                        mbuf.ptr + 8 * (n + cl.order.size), n_rec, fin.ptr, False, st)
            else:
                engine.moments_combine_segments(ctx, parts.ptr, mbuf.ptr + 8 * n,
                                                mbuf.ptr + 8 * (n + cl.order.size), n_rec, fin.ptr, st)
            keep = [mbuf, lbuf, parts, meta, lists]
        self._grouped_path = "cols" if done else "walk"
        if part and not self._components:
            # the value and its mask on the device: 2 to 9 bytes per record come back instead of 32
            stat = gs["stat"]
            vdt = engine.format_dtype(ds.dtype, stat)
            vbuf = DeviceBuffer(ctx, n_rec * (vdt.itemsize + 1))
            engine.format_partials(ctx, ds.dtype, fin.ptr, n_rec, stat, vbuf.ptr, vbuf.ptr + n_rec * vdt.itemsize,
                                   None, st)
            val = np.empty(n_rec, dtype=vdt)
            msk = np.empty(n_rec, dtype=np.uint8)
            ctx.d2h(val, vbuf.ptr, st)
            ctx.d2h(msk, vbuf.ptr + n_rec * vdt.itemsize, st)
            ctx.synchronize(st)
            del keep
            msk = msk.astype(bool)
            val[msk] = 0   # (a group that counts nothing holds no value: 0 under the mask, as an empty query gives)
            return np.ma.MaskedArray(val.reshape(rshape), mask=msk.reshape(rshape))
        final = np.zeros(n_rec, dtype=rdt)
        ctx.d2h(final, fin.ptr, st)
        ctx.synchronize(st)
        del keep
        # (the dense kernel's records lie group-major over the kept outputs: the reduced dims lead the
        # kept ones and have extent 1 but for `along`, so that is C order over the result's shape too)
        return self._format_grouped(final.reshape(rshape))

    def _format_grouped(self, parts):
        """The result of a grouped query from its records (grouped.finalize),
        or its components in :meth:`_format_moments`' form (min / max / sum:
        the whole partial records' ``sum``, ``min``, ``max`` and ``n``)."""
        stat = self._grouped["stat"]
        if stat in grouped.PARTIAL_STATS:
            if not self._components:
                return grouped.finalize(parts, stat, self._ddof, dtype=self.ds.dtype)
            empty = parts["count"] == 0
            out = {"sum": grouped.finalize(parts, "sum")}   # (the record's own 8-byte sum)
            for name in ("min", "max"):
                out[name] = grouped.finalize(parts, name, dtype=self.ds.dtype)
            out["n"] = np.ma.MaskedArray(np.ascontiguousarray(parts["count"]), mask=np.zeros(parts.shape, dtype=bool))
            return out
        if self._components:
            empty = parts["count"] == 0
            return {"mean": np.ma.MaskedArray(np.ascontiguousarray(parts["mean"]), mask=empty),
                    "m2": np.ma.MaskedArray(np.ascontiguousarray(parts["m2"]), mask=empty),
                    "n": np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                           mask=np.zeros(parts.shape, dtype=bool))}
        return grouped.finalize(parts, self._grouped["stat"], self._ddof)

    # -- histogram ------------------------------------------------------------------
    def _auto_range(self, index, compressor, filters):
        """``range=None``: the unmasked min and max of the selection as float64,
        from a min and a max query over every axis through :meth:`_reduce` (a
        resident variable's plan cache serves them); ``(0.0, 1.0)`` when nothing
        is unmasked.  ValueError when either is not finite."""
        ds = self.ds
        saved = (self._method, self._components)
        axes = tuple(range(ds.ndim))
        vals = []
        try:
            self._components = False
            for m in ("min", "max"):
                self._method = m
                res, cache_key = _MISS, None
                if self.resident:
                    ikey = _index_key(index)
                    if ikey is not None:
                        cache_key = (ikey, axes, _missing_key(self.missing))
                        res = self._cached_query(cache_key)
                if res is _MISS:
                    res = self._reduce(OrthogonalIndexer(index, ds.shape, ds.chunks), compressor, filters, axes,
                                       cache_key)
                vals.append(res)
        finally:
            self._method, self._components = saved
        if any(np.ma.getmaskarray(v).all() for v in vals):
            return 0.0, 1.0
        lo, hi = (float(np.asarray(np.ma.getdata(v), dtype=np.float64).reshape(-1)[0]) for v in vals)
        if not (np.isfinite(lo) and np.isfinite(hi)):
            raise ValueError(f"autodetected range of [{lo}, {hi}] is not finite")
        return lo, hi

    def _reduce_hist(self, index, indexer, compressor, filters, axes):
        """histogram: every chunk adds its counts straight into the final
        table, one int64 row of ``n_bins + 3`` slots per output
        (pyas_hist_axes), so there are no per-chunk records and no combine.  A
        full reduction adds into row 0; a partial one looks each chunk-local
        output's row up in a host-built map, for box and general queries
        alike."""
        h = self._hist
        n_bins = h["n"]
        slots = n_bins + 3
        final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        n_final = int(np.prod(final_shape))
        nbytes = n_final * slots * 8
        if nbytes > histogram.TABLE_CAP_BYTES:
            raise ValueError(f"histogram table of {n_final} outputs x ({n_bins} + 3) slots takes {nbytes} bytes, "
                             f"above the cap of {histogram.TABLE_CAP_BYTES} bytes")
        e = h["edges"]
        if e is None:
            e = histogram.edges(n_bins, self._auto_range(index, compressor, filters))
        tab = np.zeros((n_final, slots), dtype=np.int64)
        cp = self._count_plan(indexer, compressor, filters, axes)
        if cp is None:
            return self._format_hist(tab.reshape(final_shape + (slots,)), e)
        ctx, st, plan, axes_mask, off_ptr, idx_ptr, keep = cp
        ebuf = DeviceBuffer(ctx, e.nbytes)
        ctx.h2d(ebuf.ptr, e, st)
        tbuf = DeviceBuffer(ctx, nbytes)
        engine.hist_reset(ctx, tbuf.ptr, n_final, n_bins, st)
        uniform = (e[0], n_bins / (e[-1] - e[0])) if h["uniform"] else None
        keep += [ebuf, tbuf]
        engine.hist_axes(ctx, plan.batch, plan.mask_up.struct, ebuf.ptr, n_bins, uniform, axes_mask, off_ptr, idx_ptr,
                         tbuf.ptr, st)
        ctx.d2h(tab, tbuf.ptr, st)
        ctx.synchronize(st)
        del keep
        return self._format_hist(tab.reshape(final_shape + (slots,)), e)

    def _count_plan(self, indexer, compressor, filters, axes):
        """What a counting query (histogram, quantile) launches over: the
        query's chunks on the device, their plan (:meth:`_query_plan`) and the
        map from each chunk-local output to its table row.  ``(ctx, stream,
        plan, axes_mask, out_offsets_ptr, out_index_ptr, keep)``, the two
        pointers None for a full reduction (one row), ``keep`` the buffers to
        hold until the stream is synchronised; None when the query selects
        nothing."""
        ds = self.ds
        q = self._query_plan(indexer, compressor, filters, axes)
        if q.empty:
            return None
        if len(axes) == ds.ndim:
            return q.ctx, q.st, q.plan, q.axes_mask, None, None, q.keep
        # chunk-local output (C order over the kept selected dims) -> final output
        if q.dims is not None:
            idx = np.indices([len(p) for p in q.dims]).reshape(ds.ndim, q.n)
            all_projs = ([q.dims[d][idx[d][k]] for d in range(ds.ndim)] for k in range(q.n))
        else:
            all_projs = (projs for _, projs in q.chunk_list)
        out_off, f_all = _chunk_outputs(all_projs, axes, q.final_shape)
        meta = np.concatenate([out_off[:-1], f_all])
        mbuf = DeviceBuffer(q.ctx, meta.nbytes)
        q.ctx.h2d(mbuf.ptr, meta, q.st)
        return q.ctx, q.st, q.plan, q.axes_mask, mbuf.ptr, mbuf.ptr + 8 * q.n, q.keep + [mbuf]

    def _format_hist(self, tab, e):
        """The int64 counts of a histogram query from its table rows (counts,
        below, above, nan), or its components."""
        n_bins = e.size - 1
        counts = np.ascontiguousarray(tab[..., :n_bins])
        if self._components:
            return {"counts": counts, "bin_edges": np.array(e, dtype=np.float64),
                    "n": tab.sum(axis=-1), "below": np.ascontiguousarray(tab[..., n_bins]),
                    "above": np.ascontiguousarray(tab[..., n_bins + 1]),
                    "nan": np.ascontiguousarray(tab[..., n_bins + 2])}
        return counts

    # -- quantile -------------------------------------------------------------------
    def _reduce_select(self, indexer, compressor, filters, axes):
        """quantile: a radix select per output over the keys of its unmasked
        elements (quantile.keys), most significant digit first.  Every pass
        counts one digit into table rows of ``2^bits + 3`` slots
        (pyas_select_axes: the histogram's launch with the digit rule) and a
        small kernel extends each row's prefix by the digit that holds its
        rank (pyas_select_step).  The first pass is shared by the query; its
        per-row ``n`` and ``nan`` come back (pyas_select_totals) and set the
        ranks (quantile.ranks).  Each distinct vector of ranks is a chain that
        runs the remaining passes with its own prefixes; the final prefixes
        (the keys of the order statistics) are all that is copied back.  No
        table travels to the host."""
        ds = self.ds
        qs, method = self._quant["q"], self._quant["method"]
        qf = qs.reshape(-1)
        final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        n_final = int(np.prod(final_shape))
        bits = quantile.fit_bits(max(n_final, 1), histogram.TABLE_CAP_BYTES)
        width = quantile.key_width(ds.dtype)
        passes = quantile.digits(width, bits)
        tot = np.zeros((n_final, 2), dtype=np.int64)
        self._select_stats = {"bits": bits, "passes": 0, "chains": 0}
        cp = self._count_plan(indexer, compressor, filters, axes)
        if cp is None:
            return self._format_select(tot, None, final_shape)
        ctx, st, plan, axes_mask, off_ptr, idx_ptr, keep = cp
        tbuf = DeviceBuffer(ctx, n_final * ((1 << bits) + 3) * 8)
        totbuf = DeviceBuffer(ctx, tot.nbytes)
        keep += [tbuf, totbuf]
        launched = 0

        def count(prefix_ptr, shift, b):
            nonlocal launched
            engine.hist_reset(ctx, tbuf.ptr, n_final, 1 << b, st)
            engine.select_axes(ctx, plan.batch, plan.mask_up.struct, prefix_ptr, shift, b, axes_mask, off_ptr, idx_ptr,
                               tbuf.ptr, st)
            launched += 1

        shift0, b0 = passes[0]
        count(None, shift0, b0)
        engine.select_totals(ctx, tbuf.ptr, n_final, b0, totbuf.ptr, st)
        ctx.d2h(tot, totbuf.ptr, st)
        ctx.synchronize(st)
        # ranks among each row's non-NaN elements (a row with a NaN gives NaN whatever its ranks select)
        h, r_lo, r_hi = quantile.ranks((tot[:, 0] - tot[:, 1])[:, None], qf[None, :], method)
        chains = {}                      # rank vector -> its position among the chains
        col_lo, col_hi = [], []
        for j in range(qf.size):
            for cols, r in ((col_lo, r_lo), (col_hi, r_hi)):
                cols.append(chains.setdefault(np.ascontiguousarray(r[:, j]).tobytes(), len(chains)))
        n_ch = len(chains)
        ranks = np.stack([np.frombuffer(k, dtype=np.int64) for k in chains]) if n_ch else np.zeros((0, n_final), np.int64)
        work = np.concatenate([ranks.reshape(-1), np.zeros(n_ch * n_final, dtype=np.int64)])
        wbuf = DeviceBuffer(ctx, max(work.nbytes, 16))   # every chain's ranks, then every chain's prefixes (zero)
        keep.append(wbuf)
        ctx.h2d(wbuf.ptr, work, st)
        rank_ptr = [wbuf.ptr + 8 * n_final * c for c in range(n_ch)]
        pre_ptr = [wbuf.ptr + 8 * n_final * (n_ch + c) for c in range(n_ch)]
        for c in range(n_ch):            # every chain takes its first digit from the shared table
            engine.select_step(ctx, tbuf.ptr, n_final, b0, rank_ptr[c], pre_ptr[c], None, st)
        for c in range(n_ch):
            for shift, b in passes[1:]:
                count(pre_ptr[c], shift, b)
                engine.select_step(ctx, tbuf.ptr, n_final, b, rank_ptr[c], pre_ptr[c], None, st)
        out = np.zeros((n_ch, n_final), dtype=np.uint64)
        if n_ch:
            ctx.d2h(out, pre_ptr[0], st)
        ctx.synchronize(st)
        del keep
        self._select_stats = {"bits": bits, "passes": launched, "chains": n_ch}
        vals = quantile.values(out, ds.dtype).astype(np.float64)
        return self._format_select(tot, quantile.finalize(vals[col_lo].T, vals[col_hi].T, h, method), final_shape)

    def _format_select(self, tot, res, final_shape):
        """The float64 masked result of a quantile query (rows x q) from its
        per-row ``(n, nan)`` and interpolated values, or its components."""
        qs = self._quant["q"]
        n, nan = tot[:, 0], tot[:, 1]
        if res is None:
            res = np.zeros((tot.shape[0], qs.size), dtype=np.float64)
        res = np.where((nan > 0)[:, None], np.nan, res)
        res = np.where((n == 0)[:, None], 0.0, res)
        shape = final_shape + qs.shape
        out = np.ma.MaskedArray(np.ascontiguousarray(res.reshape(shape)),
                                mask=np.ascontiguousarray(np.broadcast_to((n == 0)[:, None], res.shape).reshape(shape)))
        if self._components:
            return {"quantile": out, "n": np.ascontiguousarray(n.reshape(final_shape)),
                    "nan": np.ascontiguousarray(nan.reshape(final_shape))}
        return out

    # -- weighted mean / sum ------------------------------------------------------
    def _weight_tables(self, coords, weights=None):
        """pyas_weights of this query (``weights``: of a second-moment query's
        keyword) for the chunks at ``coords``: the pool (a
        run of 1.0 for the dims without weights, then each weighted dim's
        vector, zero-padded to whole chunks so that every factor of an edge
        chunk is readable) and each chunk's origin in it."""
        ds = self.ds
        weights = self._weights if weights is None else weights
        coords = np.asarray(coords, dtype=np.int64).reshape(-1, ds.ndim)
        parts, pos = [np.ones(max(ds.chunks), dtype=np.float64)], max(ds.chunks)
        origin = np.zeros((len(coords), _lib.MAX_DIMS), dtype=np.int64)
        for d in sorted(weights):
            padded = np.zeros(-(-ds.shape[d] // ds.chunks[d]) * ds.chunks[d], dtype=np.float64)
            padded[:ds.shape[d]] = weights[d]
            origin[:, d] = pos + coords[:, d] * ds.chunks[d]
            parts.append(padded)
            pos += padded.size
        if pos >= 2 ** 31:
            raise NotImplementedError("weight vectors of 2^31 entries or more")
        return np.concatenate(parts), origin.astype(np.int32)

    def _reduce_weighted(self, indexer, compressor, filters, axes):
        """mean / sum with weights: per-chunk count / sum w / sum w x records
        (pyas_wsum_axes) added up in the orders of :meth:`_reduce_records`."""
        q = self._query_plan(indexer, compressor, filters, axes)
        if q.empty:
            return self._format_weighted(np.zeros(q.final_shape, dtype=engine.wsum_dtype))
        ctx, st = q.ctx, q.st
        wpool, worigin = self._weight_tables(q.coords)
        wbuf = DeviceBuffer(ctx, wpool.nbytes + worigin.nbytes)
        ctx.h2d(wbuf.ptr, wpool, st)
        ctx.h2d(wbuf.ptr + wpool.nbytes, worigin, st)

        def launch(off_ptr, out_ptr):
            engine.wsum_axes(ctx, q.plan.batch, q.plan.mask_up.struct, wbuf.ptr, wbuf.ptr + wpool.nbytes, q.axes_mask,
                             off_ptr, out_ptr, st)
        fin, keep = self._reduce_records(q, axes, _lib.WSUM_NBYTES, launch, engine.wsum_combine_segments,
                                         engine.wsum_combine_grid)
        return self._format_weighted(self._records_back(q, fin, keep, engine.wsum_dtype))

    def _reduce_wmoments(self, indexer, compressor, filters, axes):
        """var / std / cov / corr with weights=: per-chunk count / sw / sw2 /
        means / m2s / cxy records (pyas_wcomoments_axes; cov / corr: one plan
        per side, over the same chunk list and selections) merged with the
        weighted Chan formula in the orders of :meth:`_reduce_records`."""
        q = self._query_plan(indexer, compressor, filters, axes, pair=self._co)
        if q.empty:
            return self._format_wmoments(np.zeros(q.final_shape, dtype=engine.wcomoments_dtype))
        ctx, st = q.ctx, q.st
        wpool, worigin = self._weight_tables(q.coords, self._mweights)
        wbuf = DeviceBuffer(ctx, wpool.nbytes + worigin.nbytes)
        ctx.h2d(wbuf.ptr, wpool, st)
        ctx.h2d(wbuf.ptr + wpool.nbytes, worigin, st)
        by, my = (q.plan_y.batch, q.plan_y.mask_up.struct) if self._co is not None else (None, None)

        def launch(off_ptr, out_ptr):
            engine.wcomoments_axes(ctx, q.plan.batch, q.plan.mask_up.struct, by, my, wbuf.ptr,
                                   wbuf.ptr + wpool.nbytes, q.axes_mask, off_ptr, out_ptr, st)
        fin, keep = self._reduce_records(q, axes, _lib.WCOMOMENTS_NBYTES, launch, engine.wcomoments_combine_segments,
                                         engine.wcomoments_combine_grid)
        return self._format_wmoments(self._records_back(q, fin, keep, engine.wcomoments_dtype))

    def _format_wmoments(self, parts):
        """The float64 result of a weighted var / std / cov / corr query from
        its combined records (wmoments.finalize_*), or its components."""
        co = self._method in ("cov", "corr")
        if self._components:
            empty = parts["count"] == 0
            names = {"mean_x": "mean_x", "mean_y": "mean_y", "m2_x": "m2_x", "m2_y": "m2_y", "cxy": "cxy"} if co \
                else {"mean": "mean_x", "m2": "m2_x"}
            names.update(sum_of_weights="sw", sum_of_weights2="sw2")
            out = {name: np.ma.MaskedArray(np.ascontiguousarray(parts[field]), mask=empty)
                   for name, field in names.items()}
            out["n"] = np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                         mask=np.zeros(parts.shape, dtype=bool))
            return out
        if self._method == "corr":
            return wmoments.finalize_corr(parts)
        if co:
            return wmoments.finalize_cov(parts, self._ddof)
        return wmoments.finalize_var(parts, self._ddof, std=self._method == "std")

    def _format_moments(self, parts):
        """The float64 result of a var / std query from its combined records
        (moments.finalize), or its components."""
        if self._components:
            empty = parts["count"] == 0
            return {"mean": np.ma.MaskedArray(np.ascontiguousarray(parts["mean"]), mask=empty),
                    "m2": np.ma.MaskedArray(np.ascontiguousarray(parts["m2"]), mask=empty),
                    "n": np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                           mask=np.zeros(parts.shape, dtype=bool))}
        return moments.finalize(parts, self._ddof, std=self._method == "std")

    def _format_comoments(self, parts):
        """The float64 result of a cov / corr query from its combined records
        (comoments.finalize_cov / finalize_corr), or its components."""
        if self._components:
            empty = parts["count"] == 0
            out = {name: np.ma.MaskedArray(np.ascontiguousarray(parts[name]), mask=empty)
                   for name in ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")}
            out["n"] = np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                         mask=np.zeros(parts.shape, dtype=bool))
            return out
        if self._method == "corr":
            return comoments.finalize_corr(parts)
        return comoments.finalize_cov(parts, self._ddof)

    def _format_weighted(self, parts):
        """The float64 result of a weighted mean / sum query from its combined
        records (weighted.finalize), or its components."""
        if self._components:
            empty = parts["count"] == 0
            out = {"sum": np.ma.MaskedArray(np.ascontiguousarray(parts["swx"]), mask=empty),
                   "n": np.ma.MaskedArray(np.ascontiguousarray(parts["count"]),
                                          mask=np.zeros(parts.shape, dtype=bool))}
            if self._method == "mean":
                out["sum_of_weights"] = np.ma.MaskedArray(np.ascontiguousarray(parts["sw"]), mask=empty)
            return out
        return weighted.finalize(parts, mean=self._method == "mean")

    def _tie_which(self) -> int:
        """1 / 2 when the query's min / max of a float variable must give
        NumPy's sign of a zero extreme (pyas_tie_*), else 0."""
        if self.ds.dtype.kind != "f":
            return 0
        return {"min": 1, "max": 2}.get(self._method, 0)

    def _total(self, plan, st, layer_base=0, n_layers=None, keys=None):
        """Full reduction of the plan's chunks: the combined partial.  For
        min/max of a float variable the chunk partials are kept so that a
        zero extreme gets NumPy's sign: per chunk over its elements
        (storage.py:99-100, pyas_tie_chunks), then over the per-chunk values
        in the `out` array's C order (active.py:594, pyas_tie_segments);
        level 1 scans only the two chunks level 2 can pick
        (pyas_tie_chunks_total).
        Under a group the plan holds this rank's chunks, the first at
        position ``layer_base`` of the ``n_layers`` in the query, and the
        level-2 keys go to ``keys`` (a host list) for pyas_tie_finalize
        after the exchange."""
        which = self._tie_which()
        plan.launch(st, chunk_partials=bool(which))
        if which:
            ctx, dt = plan.ctx, self.ds.dtype
            n_all = plan.n_chunks if n_layers is None else int(n_layers)
            # level 1 only on the chunks the level-2 keys can pick (positions
            # decide which zero wins; the two candidates' signs are then exact)
            try:
                engine.tie_chunks_total(ctx, plan.batch, plan.mask_up.struct, plan.tie_geom(), which,
                                        plan.chunk_partials.ptr, int(layer_base), max(n_all, 1), st)
            except NotImplementedError as e:
                if keys is not None:
                    raise
                _sign_fallback(e)
                return plan.read_total(st)
            kbuf = None
            if keys is not None:
                kbuf = DeviceBuffer(ctx, 16)
                engine.tie_keys_reset(ctx, kbuf.ptr, 1, st)
            # `out` is one coordinate per chunk and every dim reduced: one call of n_all
            engine.tie_segments(ctx, dt, plan.chunk_partials.ptr, None, None, 1, plan.n_chunks, int(layer_base),
                                max(n_all, 1), which, plan.total.ptr, kbuf.ptr if kbuf else None, st)
            if kbuf is not None:
                host = np.zeros(2, dtype=np.uint64)
                ctx.d2h(host, kbuf.ptr, st)
                ctx.synchronize(st)
                keys.append(host)
        return plan.read_total(st)

    def _reduce_axes_zs(self, ctx, st, plan, axes_mask, obuf_ptr, parts_ptr, prec, zs_ok1) -> bool:
        """pyas_reduce_axes_ex into records; with PYAS_REC_ZERO_SIGN when
        the query is a min/max whose level-1 zero sign the walk can key
        (``zs_ok1``).  Returns whether it did (then pyas_tie_chunks is not
        needed)."""
        if zs_ok1 and self._tie_which() and prec in (_lib.REC_MIN, _lib.REC_MAX):
            try:
                engine.reduce_axes(ctx, plan.batch, plan.mask_up.struct, axes_mask, obuf_ptr, parts_ptr, st,
                                   rec=prec | _lib.REC_ZERO_SIGN)
                return True
            except NotImplementedError:
                pass   # another layout: the scan pass keys the sign
        # every chunk whole or a box the dense launch takes: no generic walk
        # every chunk whole or a box the dense launch takes: no generic walk;
        # no chunk of the dense launch's: no dense launch
        dense = _lib.REC_DENSE_ONLY if prec and plan.dense_boxes() else \
            _lib.REC_GENERIC_ONLY if prec and plan.no_dense_boxes() else 0
        engine.reduce_axes(ctx, plan.batch, plan.mask_up.struct, axes_mask, obuf_ptr, parts_ptr, st, rec=prec | dense)
        return False

    def _tie_grid(self, ctx, st, plan, rec, keys_ptr=None):
        """NumPy's sign of the zero min/max outputs of a partial-axis box
        query (``rec``: _grid_partials' record): per chunk output
        (storage.py:99-100), then over the chunk layers of the `out` array
        (active.py:594)."""
        which = self._tie_which()
        if not which:
            return
        t = rec["tie"]
        if t.get("fused"):   # the fold wrote NumPy's sign itself (elementwise at both levels)
            return
        dt = self.ds.dtype
        geom = plan.tie_geom()
        if rec["folded"]:   # no per-chunk partials: per chunk output flags
            if t.get("flags") is None:
                t["flags"] = DeviceBuffer(ctx, max(t["n_parts"], 1))
            engine.tie_chunk_flags(ctx, plan.batch, plan.mask_up.struct, geom, rec["axes_mask"], which,
                                   rec["obuf"].ptr, rec["fin"].ptr, rec["n_final"], t["flags"].ptr, st)
            engine.tie_grid(ctx, dt, rec["g"], None, t["flags"].ptr, t["lr"], which, rec["fin"].ptr, keys_ptr, st)
        else:   # per-chunk partials: compact records of the method (pyas_reduce_axes_ex)
            pw = which | (_lib.TIE_REC if rec.get("rec") else 0)
            if rec.get("zs2") and keys_ptr is None:   # walk and combine keyed both levels
                return
            if rec.get("zs1"):   # the walk keyed level 1 itself: only the `out` level
                engine.tie_grid(ctx, dt, rec["g"], rec["parts"].ptr, None, t["lr"], pw, rec["fin"].ptr, keys_ptr, st)
                return
            try:
                engine.tie_chunks(ctx, plan.batch, plan.mask_up.struct, geom, rec["axes_mask"], pw,
                                  rec["obuf"].ptr, rec["parts"].ptr, st)
            except NotImplementedError as e:
                if keys_ptr is not None:
                    raise
                _sign_fallback(e)
                return
            engine.tie_grid(ctx, dt, rec["g"], rec["parts"].ptr, None, t["lr"], pw, rec["fin"].ptr, keys_ptr,
                            st)

    def _exchange(self, final, keys=None, lr=1):
        """All-gather the per-rank partial grids (RCCL for an nccl group,
        else over the group's CPU backend) and fold them in rank order on
        the device (pyas_combine_segments).  ``keys``: this rank's zero-sign
        keys (2 x n uint64), gathered in the same collective and combined
        by pyas_tie_finalize, so a zero min/max carries NumPy's sign over
        the whole `out` array (active.py:594).  Every rank gets the result."""
        import torch
        import torch.distributed as dist
        world = dist.get_world_size(self.group)
        which = self._tie_which() if keys is not None else 0
        n = final.size
        ctx = get_context(self.device)
        st = ctx.thread_stream()
        if world == 1 and not which:
            return final
        dev = torch.device("cuda", torch.cuda.current_device()) \
            if dist.get_backend(self.group) == "nccl" else torch.device("cpu")
        blob = np.ascontiguousarray(final).view(np.uint8).reshape(-1)
        if which:
            blob = np.concatenate([blob, np.ascontiguousarray(keys, dtype=np.uint64).view(np.uint8)])
        t = torch.from_numpy(blob.copy()).to(dev)
        parts = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(parts, t, group=self.group)
        host = [p.cpu().numpy() for p in parts]
        gathered = np.concatenate([h[:final.nbytes] for h in host]).view(final.dtype)
        gkeys = np.concatenate([h[final.nbytes:] for h in host]).view(np.uint64) if which else None
        index = (np.arange(world, dtype=np.int64)[None, :] * n
                 + np.arange(n, dtype=np.int64)[:, None]).reshape(-1)
        seg = np.arange(n + 1, dtype=np.int64) * world
        gbuf = DeviceBuffer(ctx, gathered.nbytes)
        ctx.h2d(gbuf.ptr, gathered, st)
        meta = np.concatenate([index, seg])
        mbuf = DeviceBuffer(ctx, meta.nbytes)
        ctx.h2d(mbuf.ptr, meta, st)
        fin = DeviceBuffer(ctx, max(n, 1) * _lib.PARTIAL_NBYTES)
        engine.combine_segments(ctx, self.ds.dtype, gbuf.ptr, mbuf.ptr, mbuf.ptr + 8 * index.size, n,
                                fin.ptr, False, st)
        if which:
            kb = DeviceBuffer(ctx, gkeys.nbytes)
            ctx.h2d(kb.ptr, gkeys, st)
            engine.tie_finalize(ctx, self.ds.dtype, kb.ptr, n, world, lr, which, fin.ptr, st)
        out = np.zeros(n, dtype=final.dtype)
        ctx.d2h(out, fin.ptr, st)
        ctx.synchronize(st)
        return out

    def _grid_combine(self, ctx, st, plan, grid, axes, final_shape):
        """Partial axes over a box query, every chunk local."""
        return self._grid_partials(ctx, st, plan, grid, axes, final_shape, 0, plan.n_chunks,
                                   formatted=True)

    def _grid_partials(self, ctx, st, plan, grid, axes, final_shape, lo, hi, formatted=False, rec=None,
                       keys=None):
        """Per-chunk partial arrays of chunks [lo, hi) of the box query
        (pyas_reduce_axes over ``plan``), then pyas_combine_grid into the
        final grid; chunks outside [lo, hi) read a zeroed (count 0, neutral)
        partial region.  ``formatted``: return the formatted result
        (``_format_device``) instead of the host partials.  ``rec``: filled
        with what a replay of this query needs (_CachedQuery).  ``keys``
        (group queries): a host list that receives this rank's zero-sign
        keys of every output (pyas_tie_grid), for pyas_tie_finalize."""
        ds = self.ds
        dt = ds.dtype
        n_final = int(np.prod(final_shape))
        axes_mask = _axes_mask(axes)
        out_off, tables = grid
        n_all = out_off.size
        n_parts_all = int(tables["n_parts"])
        end = np.append(out_off, n_parts_all)
        base, top = int(end[lo]), int(end[hi])
        neutral = 0
        if lo > 0 or hi < n_all:
            neutral = int(np.diff(end).max())
        mine = out_off[lo:hi] - base
        all_off = np.full(n_all, top - base, dtype=np.int64)   # the neutral region
        all_off[lo:hi] = mine
        obuf = DeviceBuffer(ctx, mine.nbytes)
        ctx.h2d(obuf.ptr, mine, st)
        abuf = DeviceBuffer(ctx, all_off.nbytes)
        ctx.h2d(abuf.ptr, all_off, st)
        tbuf = DeviceBuffer(ctx, max(tables["blob"].nbytes, 16))
        ctx.h2d(tbuf.ptr, tables["blob"], st)
        g = _grid_struct(ds.ndim, axes, final_shape, tables, tbuf.ptr, abuf.ptr)
        fin = DeviceBuffer(ctx, max(n_final, 1) * _lib.PARTIAL_NBYTES)
        folded = fused = False
        zs_ok = self._fold_sign_ok(axes)
        if (_AXES_FOLD and lo == 0 and hi == n_all and not plan.batch.sel
                and self._whole_chunk_grid(tables, final_shape, axes)):
            try:   # one launch: chunk layers folded inside the reduction kernel
                fused = self._fold(ctx, st, plan, g, fin.ptr, zs_ok)
                folded = True
            except NotImplementedError:
                pass   # geometry without the dense column or LDS row layout: two steps
        parts = None
        prec = 0
        if not folded:
            # per-chunk outputs as compact records of the method (storage.py:98-100
            # per chunk, the sum rounded as active.py:512 stores it): 8 B per
            # output for <= 4-byte dtypes instead of the 32-B partial
            prec = engine.method_rec(self._method)
            rb = _lib.rec_nbytes(dt.itemsize, prec)
            n_parts = top - base
            parts = DeviceBuffer(ctx, max(n_parts + neutral, 1) * rb)
            if neutral:   # zero records: count 0, neutral in the combine
                zeros = np.zeros(neutral * rb, dtype=np.uint8)
                ctx.h2d(parts.ptr + n_parts * rb, zeros, st)
            # level 1 of NumPy's zero sign keyed by the per-chunk walk itself
            # where it can (PYAS_REC_ZERO_SIGN), else pyas_tie_chunks below
            zs_ok1 = zs_ok and plan.dense_boxes()
        ext = [tables["n_coords"][d] if d in axes else final_shape[d] for d in range(ds.ndim)]
        lr = zerosign.grid_lr(ext, set(axes))
        zs2 = False
        if not folded:
            zs1 = self._reduce_axes_zs(ctx, st, plan, axes_mask, obuf.ptr, parts.ptr, prec, zs_ok1)
            # level 2 in the combine where the `out` calls are elementwise
            # (group queries key it across ranks: pyas_tie_grid below)
            zs2 = self._combine_zs(ctx, st, parts.ptr, g, fin.ptr, prec, zs1 and keys is None)
        r = rec if rec is not None else {}
        if folded:
            zs_ok1 = zs1 = False
        r.update(folded=folded, g=g, fin=fin, obuf=obuf, abuf=abuf, tbuf=tbuf, parts=parts, rec=prec,
                 axes_mask=axes_mask, n_final=n_final, zs_ok=zs_ok, zs_ok1=zs_ok1, zs1=zs1, zs2=zs2,
                 tie={"lr": lr, "n_parts": n_parts_all, "flags": None, "fused": fused})
        if keys is not None and self._tie_which():
            kbuf = DeviceBuffer(ctx, max(n_final, 1) * 16)
            engine.tie_keys_reset(ctx, kbuf.ptr, n_final, st)
            self._tie_grid(ctx, st, plan, r, kbuf.ptr)
            host = np.zeros(2 * n_final, dtype=np.uint64)
            ctx.d2h(host, kbuf.ptr, st)
            ctx.synchronize(st)
            keys.append(host)
        else:
            self._tie_grid(ctx, st, plan, r)
        if formatted:
            return self._format_device(ctx, st, fin, n_final, final_shape)
        final = np.zeros(n_final, dtype=engine.partial_dtype(dt))
        ctx.d2h(final, fin.ptr, st)
        ctx.synchronize(st)
        return final

    def _combine_zs(self, ctx, st, parts_ptr, g, fin_ptr, prec, keyed) -> bool:
        """pyas_combine_grid of the per-chunk records; ``keyed`` (level 1
        keyed by the walk): level 2 of NumPy's zero sign keyed in the same
        launch, for `out` calls of any length.  Returns whether it was."""
        dt = self.ds.dtype
        which = self._tie_which() if keyed else 0
        if which:
            try:
                engine.combine_grid(ctx, dt, parts_ptr, g, fin_ptr, True, st, rec=prec, zero_sign=which)
                return True
            except NotImplementedError:
                pass
        engine.combine_grid(ctx, dt, parts_ptr, g, fin_ptr, True, st, rec=prec)
        return False

    def _fold_sign_ok(self, axes) -> bool:
        """Whether the fold may fuse NumPy's zero sign of this partial-axis
        query (PYAS_FOLD_ZERO_SIGN_*): a float variable with C-ordered chunks
        (storage.py:99-100 then reduces each chunk in the memory order the
        kernels assume) and this host's NumPy rule known.  The library
        refuses (ENOTSUP) the geometries its fold kernels cannot key."""
        ds = self.ds
        if ds.dtype.kind != "f" or getattr(ds, "order", "C") != "C":
            return False
        ctx = get_context(self.device)
        return bool(getattr(ctx, "tie_signs_exact", {}).get("f4" if ds.dtype.itemsize == 4 else "f8"))

    def _fold(self, ctx, st, plan, g, fin_ptr, zs_ok) -> bool:
        """pyas_reduce_axes_grid, with NumPy's zero sign fused in when the
        query allows it (min/max of a float variable, _fold_sign_ok) and the
        fold kernel the geometry takes can key it (the lean column fold with
        both reductions elementwise, or the LDS row fold).  Returns whether
        the sign was fused (else the zero-sign passes run)."""
        which = self._tie_which() if zs_ok else 0
        if which:
            try:
                engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, fin_ptr, True, st,
                                        zero_sign=which)
                return True
            except NotImplementedError:
                pass   # another fold kernel: the sign comes from the tie passes
        engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, fin_ptr, True, st)
        return False

    def _whole_chunk_grid(self, tables, final_shape, axes):
        """Every kept dim's output positions are whole chunks in coordinate
        order (position p -> coordinate p // chunk, local p % chunk), as
        pyas_reduce_axes_grid assumes."""
        blob = tables["blob"]
        for d, c in enumerate(self.ds.chunks):
            if d in axes:
                continue
            F = final_shape[d]
            if F != tables["n_coords"][d] * c:
                return False
            p = np.arange(F, dtype=np.int32)
            pc, pl = tables["pos_coord"][d], tables["pos_local"][d]
            if not (np.array_equal(blob[pc:pc + F], p // c) and np.array_equal(blob[pl:pl + F], p % c)):
                return False
        return True

    def _format_device(self, ctx, st, fin, n, shape, bufs=None):
        """``_format`` on the device (pyas_format_partials): only the
        result's values, mask (and counts in components mode) come back.
        ``bufs``: a dict that keeps the device result buffers for reuse."""
        dt = self.ds.dtype
        method = "sum" if (self._components and self._method == "mean") else self._method
        vdt = engine.format_dtype(dt, method)
        have = bufs.get((vdt.str, self._components)) if bufs is not None else None
        if have is None:
            have = (DeviceBuffer(ctx, max(n, 1) * vdt.itemsize), DeviceBuffer(ctx, max(n, 1)),
                    DeviceBuffer(ctx, max(n, 1) * 8) if self._components else None)
            if bufs is not None:
                bufs[(vdt.str, self._components)] = have
        vbuf, mbuf, cbuf = have
        engine.format_partials(ctx, dt, fin.ptr, n, method, vbuf.ptr, mbuf.ptr,
                               cbuf.ptr if cbuf is not None else None, st)
        vals = ctx.result_array(n, vdt)
        mask = ctx.result_array(n, np.bool_)
        ctx.d2h(vals, vbuf.ptr, st)
        ctx.d2h(mask, mbuf.ptr, st)
        if cbuf is not None:
            cnt = ctx.result_array(n, np.int64)
            ctx.d2h(cnt, cbuf.ptr, st)
        ctx.synchronize(st)
        out = np.ma.MaskedArray(vals.reshape(shape), mask=mask.reshape(shape))
        if self._components:
            nn = np.ma.MaskedArray(cnt.reshape(shape), mask=np.zeros(shape, dtype=bool))
            return {method: out, "n": nn}
        return out

    def _reduce_general(self, indexer, compressor, filters, axes):
        """Per-chunk selection objects and host-built segments: integer-
        dropped dims and vector fill/missing values."""
        ds = self.ds
        dt = ds.dtype
        chunk_list = list(indexer)
        final_shape = tuple(1 if i in axes else n for i, n in enumerate(indexer.shape))
        n_final = int(np.prod(final_shape))
        pdt = engine.partial_dtype(dt)
        if not chunk_list:
            final = np.zeros(n_final, dtype=pdt)
            return self._format(final.reshape(final_shape), final_shape)
        ctx, st, buf, offsets, fused = self._ingest([c for c, _ in chunk_list], compressor, filters)
        sels = [self._chunk_sel(projs) for _, projs in chunk_list]
        plan = ReductionPlan(ctx, dt, ds.chunks, buf.ptr, offsets, shuffle=fused, selections=sels,
                             missing=self.missing, round_to_var=True, stream=st)
        if len(axes) == ds.ndim:
            final = self._total(plan, st)
            return self._format(final.reshape(final_shape), final_shape)
        axes_mask = _axes_mask(axes)
        grid = self._grid_tables(chunk_list, axes, final_shape)
        if grid is not None:
            return self._grid_combine(ctx, st, plan, grid, axes, final_shape)
        # general case: per-chunk partial arrays, then a segmented device combine
        out_off, order, seg = _segment_meta((projs for _, projs in chunk_list), axes, final_shape)
        meta = np.concatenate([out_off[:-1], order, seg])
        mbuf = DeviceBuffer(ctx, meta.nbytes)
        ctx.h2d(mbuf.ptr, meta, st)
        prec = engine.method_rec(self._method)   # compact per-output records (see _grid_partials)
        parts = DeviceBuffer(ctx, max(int(out_off[-1]), 1) * _lib.rec_nbytes(dt.itemsize, prec))
        fin = DeviceBuffer(ctx, max(n_final, 1) * _lib.PARTIAL_NBYTES)
        engine.reduce_axes(ctx, plan.batch, plan.mask_up.struct, axes_mask, mbuf.ptr, parts.ptr, st, rec=prec)
        engine.combine_segments(ctx, dt, parts.ptr, mbuf.ptr + 8 * len(chunk_list),
                                mbuf.ptr + 8 * (len(chunk_list) + order.size), n_final, fin.ptr,
                                True, st, rec=prec)
        which = self._tie_which()
        if which:   # NumPy's zero sign: per chunk output, then over each segment's layers
            which |= _lib.TIE_REC
            engine.tie_chunks(ctx, plan.batch, plan.mask_up.struct, plan.tie_geom(), axes_mask, which, mbuf.ptr,
                              parts.ptr, st)
            ncoord = [len({cc[d] for cc, _ in chunk_list}) for d in range(ds.ndim)]
            lr = zerosign.grid_lr([ncoord[d] if d in axes else final_shape[d] for d in range(ds.ndim)], set(axes))
            engine.tie_segments(ctx, dt, parts.ptr, mbuf.ptr + 8 * len(chunk_list),
                                mbuf.ptr + 8 * (len(chunk_list) + order.size), n_final, int(np.diff(seg).max()),
                                0, lr, which, fin.ptr, None, st)
        final = np.zeros(n_final, dtype=pdt)
        ctx.d2h(final, fin.ptr, st)
        ctx.synchronize(st)
        return self._format(final.reshape(final_shape), final_shape)

    def _grid_tables(self, chunk_list, axes, final_shape):
        """``_grid_from_dims`` for a materialised chunk list, when its chunks
        are the C-ordered product of per-dim projections; else None."""
        nd = self.ds.ndim
        seen = [dict() for _ in range(nd)]
        dims = [[] for _ in range(nd)]
        idx = np.empty((len(chunk_list), nd), dtype=np.int64)
        for k, (cc, projs) in enumerate(chunk_list):
            if len(projs) != nd:
                return None
            for d in range(nd):
                p = projs[d]
                if isinstance(p.chunk_sel, (int, np.integer)):
                    return None
                a = seen[d].get(cc[d])
                if a is None:
                    a = seen[d][cc[d]] = len(dims[d])
                    dims[d].append(p)
                idx[k, d] = a
        n_coords = [len(o) for o in dims]
        if int(np.prod(n_coords)) != len(chunk_list):
            return None
        if not (np.ravel_multi_index(idx.T, n_coords) == np.arange(len(chunk_list))).all():
            return None
        return self._grid_from_dims(dims, axes, final_shape)

    @staticmethod
    def _grid_from_dims(dims, axes, final_shape):
        """Tables of ``pyas_combine_grid`` from per-dim projections (chunks =
        their C-ordered product).  Returns ``(out_off, tables)``: ``out_off[n]``
        is chunk n's offset in the partial array (its kept-dims selection, C
        order); ``tables`` holds one int32 blob with, per kept dim, position
        -> coordinate index, position -> index inside that chunk's selection
        and coordinate -> selected count (offsets in int32 units)."""
        nd = len(dims)
        n_coords = [len(p) for p in dims]
        kept = [d for d in range(nd) if d not in axes]
        counts = {d: np.array([len(p.out_pos) for p in dims[d]], dtype=np.int64) for d in kept}
        n = int(np.prod(n_coords))
        idx = np.indices(n_coords).reshape(nd, n)
        sizes = np.ones(n, dtype=np.int64)
        for d in kept:
            sizes *= counts[d][idx[d]]
        out_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64)
        parts, off = [], 0
        tables = {"n_coords": n_coords, "pos_coord": {}, "pos_local": {}, "coord_count": {},
                  "n_parts": int(sizes.sum())}
        for d in kept:
            F = final_shape[d]
            pc = np.full(F, -1, dtype=np.int32)
            pl = np.zeros(F, dtype=np.int32)
            for a, p in enumerate(dims[d]):
                o = np.asarray(p.out_pos, dtype=np.int64)
                pc[o] = a
                pl[o] = np.arange(o.size, dtype=np.int32)
            if (pc < 0).any():
                raise AssertionError("output positions not covered by the chunk projections")
            for name, arr in (("pos_coord", pc), ("pos_local", pl),
                              ("coord_count", counts[d].astype(np.int32))):
                tables[name][d] = off
                parts.append(arr)
                off += arr.size
        tables["blob"] = np.concatenate(parts) if parts else np.zeros(1, dtype=np.int32)
        return out_off, tables

    def _format(self, final, shape):
        """active.py:591-630 on combined partials."""
        dt = self.ds.dtype
        cnt = np.ascontiguousarray(final["count"]).astype(np.int64)
        if self._method in ("sum", "mean"):
            vals = final["sum"].astype(native(dt) if dt.kind == "f" else sum_dtype(dt))
        else:
            vals = final[self._method].astype(native(dt))
        out = np.ma.MaskedArray(np.ascontiguousarray(vals), mask=(cnt == 0))
        n = np.ma.MaskedArray(cnt, mask=np.zeros(shape, dtype=bool))
        if self._components:
            return {("sum" if self._method == "mean" else self._method): out, "n": n}
        if self._method == "mean":
            return out / n
        return out

    # -- method=None --------------------------------------------------------
    def _select(self, indexer, compressor, filters):
        if not any(m is not None and np.size(m) != 1 for m in self.missing):
            return self._select_scatter(indexer, compressor, filters)
        return self._select_general(indexer, compressor, filters)

    def _select_scatter(self, indexer, compressor, filters):
        """method=None over the whole query in one launch: every selected
        element is written by the device straight to its place in the
        C-ordered result (pyas_select_scatter), instead of per-chunk host
        placement at each chunk's out_selection."""
        ds = self.ds
        dt = ds.dtype
        dims = [list(d) for d in indexer.dim_indexers]
        nd = len(dims)
        n_coords = [len(p) for p in dims]
        n = int(np.prod(n_coords))
        out_shape = indexer.shape
        # output strides: C order over the kept dims, 0 for integer-dropped ones
        ostride = np.zeros(nd, dtype=np.int64)
        kept = [d for d in range(nd) if indexer.dim_indexers[d].kind != "int"]
        acc = 1
        for d in reversed(kept):
            ostride[d] = acc
            acc *= out_shape[kept.index(d)]
        ent, pos_parts, bases, pool_parts = [], [], [], []
        ppos = poolpos = 0
        for projs in dims:
            e = np.zeros((len(projs), 3), dtype=np.int32)
            b = np.zeros(len(projs), dtype=np.int32)
            for a, p in enumerate(projs):
                sl = p.chunk_sel
                if isinstance(sl, slice):
                    cnt = len(p.out_pos)
                    e[a] = (sl.start if cnt else 0, sl.step, cnt)
                    op = np.asarray(p.out_pos, dtype=np.int64)
                elif isinstance(sl, np.ndarray):
                    e[a] = (poolpos, 0, sl.size)
                    pool_parts.append(sl.astype(np.int32))
                    poolpos += sl.size
                    op = np.asarray(p.out_pos, dtype=np.int64)
                else:                                        # integer index: dropped dim
                    e[a] = (int(sl), 1, 1)
                    op = np.zeros(1, dtype=np.int64)
                b[a] = ppos
                pos_parts.append(op)
                ppos += op.size
            ent.append(e)
            bases.append(b)
        nd_native = native(dt)
        if n == 0 or int(np.prod(out_shape)) == 0:
            return np.ma.MaskedArray(np.zeros(out_shape, dtype=dt))
        idx = np.indices(n_coords).reshape(nd, n)
        table = np.zeros((n, _lib.MAX_DIMS, 3), dtype=np.int32)
        table[:, :, 1] = 1
        table[:, :, 2] = 1
        cbase = np.zeros((n, nd), dtype=np.int32)
        coords = np.zeros((n, nd), dtype=np.int64)
        for d in range(nd):
            table[:, d, :] = ent[d][idx[d]]
            cbase[:, d] = bases[d][idx[d]]
            coords[:, d] = np.array([p.chunk_ix for p in dims[d]], dtype=np.int64)[idx[d]]
        pool = np.concatenate(pool_parts) if pool_parts else np.zeros(1, dtype=np.int32)
        pos = np.concatenate(pos_parts)
        ctx, st, buf, offsets, fused = self._ingest(coords, compressor, filters)
        full = _all_full(table, ds.chunks)
        plan = ReductionPlan(ctx, dt, ds.chunks, buf.ptr, offsets, shuffle=fused,
                             sel_table=None if full else table, index_pool=None if full else pool,
                             missing=self.missing, stream=st)
        total = int(np.prod(out_shape))
        pb = DeviceBuffer(ctx, pos.nbytes)
        ctx.h2d(pb.ptr, pos, st)
        cb = DeviceBuffer(ctx, cbase.nbytes)
        ctx.h2d(cb.ptr, np.ascontiguousarray(cbase), st)
        sc = _lib.Scatter()
        sc.pos, sc.chunk_base = pb.ptr, cb.ptr
        for d in range(nd):
            sc.out_stride[d] = int(ostride[d])
        vals = ctx.result_array(total, nd_native)
        msk = ctx.result_array(total, np.uint8)
        vb = DeviceBuffer(ctx, vals.nbytes)
        mb = DeviceBuffer(ctx, msk.nbytes)
        engine.select_scatter(ctx, plan.batch, plan.mask_up.struct, sc, vb.ptr, mb.ptr, st)
        ctx.d2h(vals, vb.ptr, st)
        ctx.d2h(msk, mb.ptr, st)
        ctx.synchronize(st)
        out_vals = vals.reshape(out_shape).astype(dt, copy=False)
        out_mask = msk.reshape(out_shape).view(bool)
        if out_mask.any():
            return np.ma.MaskedArray(out_vals, mask=out_mask)
        return np.ma.MaskedArray(out_vals)

    def _select_general(self, indexer, compressor, filters):
        """method=None with vector fill/missing values (per-chunk selections)."""
        ds = self.ds
        dt = ds.dtype
        chunk_list = list(indexer)
        out_vals = np.zeros(indexer.shape, dtype=dt)
        out_mask = np.zeros(indexer.shape, dtype=bool)
        if chunk_list:
            ctx, st, buf, offsets, fused = self._ingest([c for c, _ in chunk_list], compressor, filters)
            sels = [self._chunk_sel(projs) for _, projs in chunk_list]
            plan = ReductionPlan(ctx, dt, ds.chunks, buf.ptr, offsets, shuffle=fused,
                                 selections=sels, missing=self.missing, stream=st)
            sizes = np.array([s.n_selected for s in sels], dtype=np.int64)
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
            total = int(off[-1])
            nd = native(dt)
            vals = np.zeros(max(total, 1), dtype=nd)
            msk = np.zeros(max(total, 1), dtype=np.uint8)
            ob = DeviceBuffer(ctx, off.nbytes)
            ctx.h2d(ob.ptr, off, st)
            vb = DeviceBuffer(ctx, vals.nbytes)
            mb = DeviceBuffer(ctx, msk.nbytes)
            engine.select_chunks(ctx, plan.batch, plan.mask_up.struct, ob.ptr, vb.ptr, mb.ptr, st)
            ctx.d2h(vals, vb.ptr, st)
            ctx.d2h(msk, mb.ptr, st)
            ctx.synchronize(st)
            for c, (_, projs) in enumerate(chunk_list):
                block = slice(int(off[c]), int(off[c + 1]))
                where = np.ix_(*[p.out_pos for p in projs if not isinstance(p.chunk_sel, (int, np.integer))])
                out_vals[where] = vals[block].reshape(sels[c].shape)
                out_mask[where] = msk[block].reshape(sels[c].shape).astype(bool)
        if out_mask.any():
            return np.ma.MaskedArray(out_vals, mask=out_mask)
        return np.ma.MaskedArray(out_vals)
