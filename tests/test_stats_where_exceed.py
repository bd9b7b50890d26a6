"""``Active.exceed`` on the device against NumPy.

Oracle: the orthogonal selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``, compared in float64 against the scalar or
the field's entry at the output's global index; ``n`` and ``n_true`` exact,
``sum`` and ``excess`` by ``math.fsum`` over the float64 terms (an excess term
is the one float64 subtraction the kernels make).  It shares nothing with
``pyactivestorage_amd/exceed.py``.  Sums are held to
``tests/_compare.sum_bound("float64", n_true, sum|term|)`` for every dtype (the
accumulator is float64 from the first addition), ``fraction`` and ``mean`` to
its ``kind="mean"`` form.  ``exceed_path`` is asserted in every case, so a
query that silently took the other kernel fails.

The padding of an edge chunk compares *true* (above every value for ``gt`` /
``ge``, below for ``lt`` / ``le``), so a kernel that read it would over-count.
"""
import functools
import math
import os

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import exceed
from pyactivestorage_amd.active import _RECORD_SEG, Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes
from tests._compare import assert_within, sum_bound

pytestmark = pytest.mark.gpu

OPS = ("gt", "ge", "lt", "le")
STATS = ("count", "fraction", "sum", "mean", "excess")
DTYPES = ("|i1", "|u1", "<i2", "<u2", "<i4", "<u4", "<i8", "<u8", "<f4", "<f8")
LO, HI, MID = 10, 50, 30            # the random values' range and the scalar threshold
PAD = {"gt": 100, "ge": 100, "lt": 1, "le": 1}     # true against every threshold of the range


def make_var(data, chunks, attrs=None, shuffle=False, pad=0):
    """In-memory chunked variable of ``data`` (edge chunks padded with
    ``pad``), optionally stored with the HDF5 byte shuffle."""
    dt, shape = data.dtype, data.shape
    blobs, index, pos = [], {}, 0
    for cc in np.ndindex(*[-(-s // c) for s, c in zip(shape, chunks)]):
        block = np.full(chunks, pad, dt)
        sl = tuple(slice(i * c, min((i + 1) * c, s)) for i, c, s in zip(cc, chunks, shape))
        block[tuple(slice(0, x.stop - x.start) for x in sl)] = data[sl]
        raw = block.tobytes()
        if shuffle:
            raw = np.frombuffer(raw, np.uint8).reshape(-1, dt.itemsize).T.tobytes()
        index[cc] = (pos, len(raw))
        blobs.append(raw)
        pos += len(raw)
    blob = b"".join(blobs)
    pipeline = [{"filter_id": 2, "client_data": [dt.itemsize]}] if shuffle else None
    return ChunkedVariable(name="v", shape=shape, chunks=chunks, dtype=dt, chunk_index=index, attrs=attrs or {},
                           filter_pipeline=pipeline, reader=lambda off, size: blob[off:off + size])


def by_op(x, chunks, attrs=None, shuffle=False, pad=None):
    """The variable per op: they differ in their padding only."""
    pad = pad or PAD
    hi, lo = (make_var(x, chunks, attrs, shuffle=shuffle, pad=pad[op]) for op in ("gt", "lt"))
    return {"gt": hi, "ge": hi, "lt": lo, "le": lo}


def values(shape, seed, dt="<f4"):
    """Quarter steps for floats (sums that round), integers otherwise; many
    elements equal MID, so ``gt`` and ``ge`` differ."""
    rng = np.random.default_rng(seed)
    if np.dtype(dt).kind == "f":
        x = (rng.integers(4 * LO, 4 * HI + 1, shape) / 4.0).astype(dt)
        x[rng.random(shape) < 0.1] = MID
        return x
    return rng.integers(LO, HI + 1, shape).astype(dt)


def field_for(shape, axes, masked=()):
    """A threshold per grid point of the kept dims, every one its own
    (20 .. 40.5 in half steps by global position): a wrong global index
    compares against a neighbour's threshold and changes counts.  ``masked``:
    flat positions to mask."""
    fshape = tuple(1 if d in axes else n for d, n in enumerate(shape))
    size = int(np.prod(fshape))
    t = (20.0 + (np.arange(size) * 7 % 42) / 2.0).reshape(fshape)
    if not len(masked):
        return t
    m = np.zeros(size, dtype=bool)
    m[list(masked)] = True
    return np.ma.MaskedArray(t, mask=m.reshape(fshape))


def _full_index(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    where = [k for k, s in enumerate(index) if s is Ellipsis]
    if where:
        k = where[0]
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def _ortho(a, index, skip=()):
    for d, s in enumerate(index):                   # orthogonal: one dim at a time
        if d not in skip:
            a = a[(slice(None),) * d + (s,)]
    return a


def oracle(data, attrs, index, axis, op, thr, missing=None):
    """Per output (reduced dims kept at extent 1): ``n``, ``n_true``, ``sum``,
    ``excess``, the sums of magnitudes of their terms, and ``tmask`` (the
    output's threshold is masked)."""
    nd = data.ndim
    index = _full_index(index, nd)
    axes = tuple(range(nd)) if axis is None else tuple(sorted(a % nd for a in axis))
    ys = ref.mask_missing(_ortho(data, index), missing or get_missing_attributes(attrs or {}))
    valid = ~np.ma.getmaskarray(ys)
    x = np.ma.getdata(ys).astype(np.float64)
    kept = [d for d in range(nd) if d not in axes]
    perm = kept + list(axes)
    fshape = tuple(1 if d in axes else n for d, n in enumerate(x.shape))
    n_out = int(np.prod(fshape))
    x2 = np.transpose(x, perm).reshape(n_out, -1)
    ok2 = np.transpose(valid, perm).reshape(n_out, -1)
    if np.ndim(thr) == 0:
        t, tmask = np.full(n_out, float(thr)), np.zeros(n_out, dtype=bool)
    else:                                           # the field at the kept dims' global indices
        tsel = _ortho(thr, index, skip=axes)
        t = np.ma.getdata(tsel).astype(np.float64).reshape(n_out)
        tmask = np.ma.getmaskarray(tsel).reshape(n_out).copy()
    out = {k: np.zeros(n_out, dtype=np.int64) for k in ("n", "n_true")}
    out.update({k: np.zeros(n_out) for k in ("sum", "excess", "abs_sum", "abs_excess")})
    out["tmask"] = tmask
    with np.errstate(all="ignore"):
        for i in range(n_out):
            row, ti = x2[i], t[i]
            cmp = {"gt": row > ti, "ge": row >= ti, "lt": row < ti, "le": row <= ti}[op]
            true = ok2[i] & cmp & (not tmask[i])
            out["n"][i], out["n_true"][i] = ok2[i].sum(), true.sum()
            terms = row[true]
            eterms = (terms - ti) if op in ("gt", "ge") else (ti - terms)
            for name, v in (("sum", terms), ("excess", eterms)):
                a = np.abs(v).sum()
                out["abs_" + name][i] = a
                out[name][i] = math.fsum(v) if np.isfinite(a) else v.sum()
    return {k: v.reshape(fshape) for k, v in out.items()}


def query(var, op, thr, stat, axis, index, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = a.exceed(op, thr, stat, axis=axis)[index]
    return got, a.exceed_path


def check_components(comp, o, what=""):
    assert sorted(comp) == ["excess", "n", "n_true", "sum"], what
    for k in comp:
        assert isinstance(comp[k], np.ma.MaskedArray) and not np.ma.getmaskarray(comp[k]).any(), (what, k)
        assert comp[k].shape == o["n"].shape, (what, k, comp[k].shape, o["n"].shape)
    for k in ("n", "n_true"):
        assert comp[k].dtype == np.int64 and np.array_equal(comp[k].data, o[k]), (what, k, comp[k].data, o[k])
    for k in ("sum", "excess"):
        assert comp[k].dtype == np.float64, (what, k)
        assert_within(comp[k].data, o[k], sum_bound("float64", o["n_true"], o["abs_" + k]), f"{what} {k}")


def check_stat(got, o, stat, what=""):
    n, nt = o["n"], o["n_true"]
    assert isinstance(got, np.ma.MaskedArray) and got.shape == n.shape, (what, got.shape, n.shape)
    assert got.dtype == (np.int64 if stat == "count" else np.float64), (what, got.dtype)
    wm = ((nt == 0) if stat == "mean" else (n == 0)) | o["tmask"]
    assert np.array_equal(np.ma.getmaskarray(got), wm), (what, np.ma.getmaskarray(got), wm)
    g, keep = got.data[~wm], ~wm
    with np.errstate(all="ignore"):
        if stat == "count":
            assert np.array_equal(g, nt[keep]), (what, g, nt[keep])
        elif stat == "fraction":
            assert_within(g, nt[keep] / n[keep], sum_bound("float64", n[keep], nt[keep], kind="mean"), what)
        elif stat == "mean":
            assert_within(g, o["sum"][keep] / nt[keep],
                          sum_bound("float64", nt[keep], o["abs_sum"][keep], kind="mean"), what)
        else:
            assert_within(g, o[stat][keep], sum_bound("float64", nt[keep], o["abs_" + stat][keep]), what)


def check_all(x, attrs, vars_, index, axis, thr, path, what="", ops=OPS, stats=STATS, missing=None, **kw):
    """The components and the plain result of every stat, for every op."""
    for op in ops:
        o = oracle(x, attrs, index, axis, op, thr, missing=missing)
        comp, took = query(vars_[op], op, thr, "count", axis, index, components=True, **kw)
        assert took == path, (what, op, took)
        check_components(comp, o, f"{what} {op} components")
        for stat in stats:
            got, took = query(vars_[op], op, thr, stat, axis, index, **kw)
            assert took == path, (what, op, stat, took)
            check_stat(got, o, stat, f"{what} {op} {stat}")


# -- 1. the dense column kernel ---------------------------------------------------------
DENSE = {
    # a partial last layer, items cut by the box at both ends, 3 chunk columns along the innermost dim
    "box64": ((37, 6, 136), (8, 3, 64), (slice(3, 35), slice(1, 6), slice(5, 131)), (0,)),
    # rows that are no multiple of 4 elements: predicated loads
    "box30": ((37, 6, 136), (8, 3, 30), (slice(3, 35), slice(1, 6), slice(5, 131)), (0,)),
    # 1030 rows per layer: a second staging pass of 1024 rows
    "rows1030": ((1100, 2, 8), (1030, 1, 8), Ellipsis, (0,)),
    # a leading prefix of two reduced dims
    "prefix01": ((9, 10, 40), (4, 4, 16), (slice(1, 9), slice(2, 9), slice(3, 38)), (0, 1)),
}


@functools.lru_cache(maxsize=None)
def dense_var(name):
    shape, chunks, _, _ = DENSE[name]
    x = values(shape, 100 + sorted(DENSE).index(name))
    return x, by_op(x, chunks)


@pytest.mark.parametrize("kind", ["scalar", "field"])
@pytest.mark.parametrize("name", sorted(DENSE))
def test_cols_geometry(gpu, name, kind):
    shape, _, index, axis = DENSE[name]
    x, vars_ = dense_var(name)
    thr = MID if kind == "scalar" else field_for(shape, axis)
    check_all(x, None, vars_, index, axis, thr, "cols", what=f"{name} {kind}")


# -- 2. the ten dtypes, plain, shuffled and big-endian ------------------------------------
LAYOUTS = [(dt, lay) for dt in DTYPES for lay in ("plain", "shuffled", "big")
           if not (lay == "big" and np.dtype(dt).itemsize == 1)]


@pytest.mark.parametrize("dt,layout", LAYOUTS, ids=[f"{d[1:]}-{lay}" for d, lay in LAYOUTS])
def test_dtypes(gpu, dt, layout):
    d = np.dtype(dt).newbyteorder(">") if layout == "big" else np.dtype(dt)
    shape, chunks = (10, 5, 12), (4, 3, 8)
    x = values(shape, 200 + DTYPES.index(dt), d)
    vars_ = by_op(x, chunks, shuffle=(layout == "shuffled"))
    field = field_for(shape, (0,))
    dense, walk = (slice(1, 9), slice(None), slice(2, 11)), (slice(None, None, 2), slice(None), [1, 4, 5, 10])
    for thr, ops in ((MID, ("ge", "lt")), (field, ("gt", "le"))):
        check_all(x, None, vars_, dense, (0,), thr, "cols", what=f"{d.str} {layout} dense", ops=ops,
                  stats=("count", "excess"))
        check_all(x, None, vars_, walk, (0,), thr, "walk", what=f"{d.str} {layout} walk", ops=ops,
                  stats=("count", "sum"))
    check_all(x, None, vars_, Ellipsis, None, MID, "walk", what=f"{d.str} {layout} full", ops=("gt", "le"),
              stats=("mean",))


# -- 3. the mask rules --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked_var():
    """Values every rule masks would compare true for one op or the other."""
    x = values((23, 6, 8), 33)
    x[7, 0, 0] = 1000.0                            # _FillValue: true for gt
    x[3, 0, 1] = 500.0                             # above valid_max: true for gt
    x[12, 0, 2] = 2.0                              # below valid_min: true for lt
    x[6, 0, 3] = -1000.0                           # missing_value: true for lt
    x[:, 0, 4] = 1000.0                            # a wholly masked output
    x[:, 0, 5] = 1000.0
    x[10:16, 0, 5] = [30, 40, 40, 20, 20, 30]      # masked but for six rows across a layer boundary
    x[5:11, 1, 0] = 500.0                          # a masked stretch across a layer boundary
    attrs = {"_FillValue": np.array([1000.0], "<f4"), "missing_value": np.array([-1000.0], "<f4"),
             "valid_min": np.array([8.0], "<f4"), "valid_max": np.array([400.0], "<f4")}
    pad = {"gt": 300.0, "ge": 300.0, "lt": 9.0, "le": 9.0}    # unmasked, and true
    return x, attrs, pad


def test_mask_rules(gpu):
    x, attrs, pad = masked_var()
    vars_ = by_op(x, (5, 3, 8), attrs, pad=pad)
    walk = (slice(None), slice(None), [0, 1, 2, 3, 4, 5, 7])
    for thr in (MID, field_for(x.shape, (0,))):
        check_all(x, attrs, vars_, Ellipsis, (0,), thr, "cols", what="masked")
        check_all(x, attrs, vars_, walk, (0,), thr, "walk", what="masked walk", stats=("count", "mean"))
    comp, _ = query(vars_["gt"], "gt", MID, "count", (0,), Ellipsis, components=True)
    n = comp["n"].data
    assert n[0, 0, 0] == 22 and n[0, 0, 4] == 0 and n[0, 0, 5] == 6 and n[0, 1, 0] == 17
    got, _ = query(vars_["gt"], "gt", MID, "count", (0,), Ellipsis)
    assert np.ma.getmaskarray(got)[0, 0, 4] and np.ma.getmaskarray(got).sum() == 1 and got.data[0, 0, 5] == 2
    # fill value only (mask mode: equality), and thresholds only (mask mode: range)
    for sub in ({"_FillValue": attrs["_FillValue"]}, {"valid_min": attrs["valid_min"], "valid_max": attrs["valid_max"]}):
        check_all(x, sub, by_op(x, (5, 3, 8), sub, pad=pad), Ellipsis, (0,), MID, "cols",
                  what=f"masked {sorted(sub)}", ops=("ge", "lt"), stats=("count", "sum"))
        check_all(x, sub, by_op(x, (5, 3, 8), sub, pad=pad), Ellipsis, None, MID, "walk",
                  what=f"masked full {sorted(sub)}", ops=("ge", "lt"), stats=("count", "sum"))


def test_vector_missing_value(gpu):
    """A vector ``missing_value`` (broadcast over the last dim of each chunk's
    selection) has no dense path: the walk, for partial axes and every dim.
    (Vector rules need equal selection shapes in every chunk: whole chunks.)"""
    x = values((10, 6, 10), 34)
    vec = np.array([91.0, 92.0, 93.0, 94.0, 95.0], "<f4")
    hit = np.random.default_rng(61).random(x.shape) < 0.15
    x[hit] = np.broadcast_to(np.tile(vec, 2), x.shape)[hit]
    x[:, 0, 0] = 91.0                                            # a wholly masked output
    vars_ = by_op(x, (5, 3, 5), {"missing_value": vec})
    missing = (None, np.tile(vec, 2), None, None)
    for axis in ((0,), (2,), None):
        check_all(x, None, vars_, Ellipsis, axis, 60.0, "walk", what=f"vector missing {axis}", missing=missing,
                  ops=("gt", "le"), stats=("count", "sum"))
    got, _ = query(vars_["gt"], "gt", 60.0, "count", (0,), Ellipsis)
    assert np.ma.getmaskarray(got)[0, 0, 0] and got[0, 1, 1] == 0


def test_masked_threshold_entries(gpu):
    """Nothing compares true against a masked threshold; the plain result is
    masked there and the components report ``n_true == 0``."""
    x = values((13, 6, 20), 35)
    vars_ = by_op(x, (4, 3, 8))
    field = field_for(x.shape, (0,), masked=(0, 7, 25, 119))
    listed = (slice(None), slice(None, None, 2), [0, 5, 7, 19])
    for index, path in ((Ellipsis, "cols"), ((slice(2, 12), slice(0, 5), slice(3, 20)), "cols"), (listed, "walk")):
        check_all(x, None, vars_, index, (0,), field, path, what=f"masked threshold {path}")
    comp, _ = query(vars_["gt"], "gt", field, "count", (0,), Ellipsis, components=True)
    assert comp["n"].data[0, 0, 7] == 13 and comp["n_true"].data[0, 0, 7] == 0 and comp["sum"].data[0, 0, 7] == 0.0
    got, _ = query(vars_["lt"], "lt", field, "sum", (0,), listed)
    assert got.mask[0, 0].tolist() == [True, False, True, False]           # global columns 0 and 7 of row 0
    # a one-entry field whose entry is masked: every dim reduced
    one = np.ma.MaskedArray(np.full((1, 1, 1), 30.0), mask=True)
    got, took = query(vars_["gt"], "gt", one, "count", None, Ellipsis)
    assert took == "walk" and got.shape == (1, 1, 1) and got.mask.all()
    comp, _ = query(vars_["gt"], "gt", one, "count", None, Ellipsis, components=True)
    assert comp["n"].data.item() == x.size and comp["n_true"].data.item() == 0 and comp["excess"].data.item() == 0.0
    plain = np.full((1, 1, 1), 30.0)                                        # unmasked: the scalar case
    check_all(x, None, vars_, Ellipsis, None, plain, "walk", what="one-entry field", ops=("gt",), stats=("count",))


# -- 4. the walk --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_var():
    x = values((20, 9, 14), 41)
    return x, by_op(x, (8, 4, 6))


def test_walk_strided_and_listed_kept_dims(gpu):
    x, vars_ = walk_var()
    field = field_for(x.shape, (0,))
    index = (slice(None), slice(None, None, 2), [1, 4, 5])
    check_all(x, None, vars_, index, (0,), field, "walk", what="strided listed field")
    check_all(x, None, vars_, index, (0,), MID, "walk", what="strided listed scalar", stats=("count", "excess"))
    # the field is read at the global index: shifted by one point the counts change
    o = oracle(x, None, index, (0,), "gt", field)
    shifted = np.roll(field, 1, axis=2)
    assert not np.array_equal(o["n_true"], oracle(x, None, index, (0,), "gt", shifted)["n_true"])
    # a boolean mask on a kept dim, and on the reduced dim
    keep = np.zeros(14, dtype=bool)
    keep[[0, 3, 6, 7, 13]] = True
    rows = np.arange(20) % 3 != 1
    check_all(x, None, vars_, (slice(1, 19), slice(None), keep), (0,), field, "walk", what="boolean kept",
              stats=("count", "sum"))
    check_all(x, None, vars_, (rows, slice(None), slice(None)), (0,), field, "walk", what="boolean reduced",
              stats=("count", "sum"))


@pytest.mark.parametrize("n_inner", [40, 150])
def test_walk_wave_per_output(gpu, n_inner):
    """``axis=(2,)``: a wave owns an output, with fewer and with more than 64
    reduced positions in a chunk."""
    x = values((6, 5, n_inner), 42 + n_inner)
    vars_ = by_op(x, (4, 3, n_inner))
    field = field_for(x.shape, (2,))
    for thr in (MID, field):
        check_all(x, None, vars_, Ellipsis, (2,), thr, "walk", what=f"wave {n_inner}")
    check_all(x, None, vars_, (slice(1, 6), slice(None, None, 2), slice(3, n_inner - 2)), (2,), field, "walk",
              what=f"wave {n_inner} cut", stats=("count", "excess"))


def test_walk_lane_per_output_and_grid_combine(gpu):
    """Non-prefix axes on a box: ``(1,)`` (a lane per output) and ``(0, 2)`` (a
    wave per output), both through the grid combine."""
    x, vars_ = walk_var()
    box = (slice(1, 19), slice(1, 9), slice(2, 13))
    for axis in ((1,), (0, 2), (1, 2)):
        for thr in (MID, field_for(x.shape, axis)):
            check_all(x, None, vars_, box, axis, thr, "walk", what=f"box axes {axis}")
        check_all(x, None, vars_, Ellipsis, axis, field_for(x.shape, axis), "walk", what=f"whole axes {axis}",
                  ops=("ge", "lt"), stats=("count", "sum"))


def test_walk_past_the_lds_map(gpu):
    """More than 4096 reduced positions in a chunk: no offset map."""
    x = values((70, 3, 66), 44)
    vars_ = by_op(x, (70, 2, 66))
    field = field_for(x.shape, (0, 2))
    assert 70 * 66 > 4096
    for thr in (MID, field):
        check_all(x, None, vars_, Ellipsis, (0, 2), thr, "walk", what="past the map", ops=("gt", "le"))
    check_all(x, None, vars_, (slice(1, 70), slice(None), slice(0, 65)), (0, 2), field, "walk",
              what="past the map cut", ops=("ge",), stats=("count", "sum"))
    x1, v1 = walk_var()                                           # lane per output, mapped and not
    check_all(x1, None, v1, Ellipsis, (0, 1), field_for(x1.shape, (0, 1)), "cols", what="prefix whole",
              ops=("gt",), stats=("count",))


# -- 5. every dim reduced -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_var(dt="<f4"):
    x = values((33, 65, 31), 51, dt)
    return x, by_op(x, (33, 65, 31))


FULL_INDEX = {"whole": Ellipsis,
              "run": (slice(1, 32), slice(None), slice(None)),                    # contiguous, head and tail misaligned
              "run2": (slice(4, 5), slice(3, 60), slice(None)),
              "cut": (slice(1, 32), slice(2, 64), slice(1, 30)),                  # not contiguous
              "step": (slice(None, None, 3), slice(None), [0, 7, 30])}


@pytest.mark.parametrize("name", sorted(FULL_INDEX))
def test_full_reduction(gpu, name):
    x, vars_ = full_var()
    check_all(x, None, vars_, FULL_INDEX[name], None, MID, "walk", what=f"full {name}")
    assert query(vars_["gt"], "gt", MID, "count", None, FULL_INDEX[name])[0].shape == (1, 1, 1)


def test_full_reduction_small_tiles(gpu):
    """Several tiles per chunk (and a tile boundary inside the run)."""
    x, vars_ = full_var()
    base = {k: query(vars_["gt"], "gt", MID, "count", None, FULL_INDEX[k], components=True)[0] for k in FULL_INDEX}
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        for name in sorted(FULL_INDEX):
            check_all(x, None, vars_, FULL_INDEX[name], None, MID, "walk", what=f"tiles {name}", ops=("gt", "le"))
            comp, _ = query(vars_["gt"], "gt", MID, "count", None, FULL_INDEX[name], components=True)
            for k in ("n", "n_true"):
                assert np.array_equal(comp[k].data, base[name][k].data), (name, k)
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)


def test_full_reduction_two_fold_levels(gpu):
    """More chunks than one fold segment: the records fold in two levels."""
    x = values((9, 5, 24), 52)
    vars_ = by_op(x, (2, 2, 5))
    assert 5 * 3 * 5 > _RECORD_SEG
    check_all(x, None, vars_, Ellipsis, None, MID, "walk", what="two levels")
    check_all(x, None, vars_, (slice(1, 9), slice(None), slice(2, 23)), None, 25.5, "walk", what="two levels cut",
              ops=("ge", "lt"))


# -- 6. edge values ---------------------------------------------------------------------------
def test_equal_to_the_threshold_and_zeros(gpu):
    x = np.full((9, 4, 8), 30.0, "<f4")
    x[::2] = 31.0
    x[1, 0, 0] = 29.0
    vars_ = by_op(x, (4, 4, 8))
    for index, axis, path in ((Ellipsis, (0,), "cols"), (Ellipsis, (2,), "walk"), (Ellipsis, None, "walk")):
        check_all(x, None, vars_, index, axis, 30.0, path, what=f"equal {axis}")
    c = {op: query(vars_[op], op, 30.0, "count", (0,), Ellipsis)[0].data[0, 0, 0] for op in OPS}
    assert c == {"gt": 5, "ge": 8, "lt": 1, "le": 4}
    # -0.0 against a 0.0 threshold, and 0.0 against -0.0: equal, so only ge and le are true
    z = np.zeros((6, 2, 8), "<f8")
    z[::2] = -0.0
    zv = by_op(z, (4, 2, 8), pad={"gt": 5.0, "ge": 5.0, "lt": -5.0, "le": -5.0})
    for thr in (0.0, -0.0):
        for axis, path in (((0,), "cols"), ((1,), "walk")):
            check_all(z, None, zv, Ellipsis, axis, thr, path, what=f"zeros {thr!r} {axis}")
        c = {op: query(zv[op], op, thr, "count", (0,), Ellipsis)[0].data[0, 0, 0] for op in OPS}
        assert c == {"gt": 0, "ge": 6, "lt": 0, "le": 6}, (thr, c)


@pytest.mark.parametrize("dt", ["<f4", "<f8"])
def test_nan_and_infinite_elements(gpu, dt):
    """A NaN is unmasked but never true; an infinity is true where it
    compares so, and its sums are infinite or NaN exactly as NumPy's."""
    x = values((10, 3, 8), 62, dt)
    x[2, 0, 0] = x[7, 0, 0] = np.nan
    x[:, 0, 1] = np.nan                            # every element NaN: n == 10, nothing true
    x[3, 0, 2] = np.inf
    x[4, 0, 3] = -np.inf
    x[1, 0, 4], x[8, 0, 4] = np.inf, -np.inf
    x[5, 1, 0], x[6, 1, 0] = np.inf, np.inf
    vars_ = by_op(x, (4, 3, 8))
    for thr in (MID, field_for(x.shape, (0,))):
        check_all(x, None, vars_, Ellipsis, (0,), thr, "cols", what=f"nan inf {dt}")
        check_all(x, None, vars_, (slice(None), slice(None), [0, 1, 2, 3, 4, 6]), (0,), thr, "walk",
                  what=f"nan inf walk {dt}")
    check_all(x, None, vars_, Ellipsis, None, MID, "walk", what=f"nan inf full {dt}")
    comp, _ = query(vars_["gt"], "gt", MID, "count", (0,), Ellipsis, components=True)
    assert comp["n"].data[0, 0, 0] == 10 and comp["n"].data[0, 0, 1] == 10 and comp["n_true"].data[0, 0, 1] == 0
    assert comp["sum"].data[0, 0, 2] == np.inf and comp["excess"].data[0, 0, 2] == np.inf
    got, _ = query(vars_["gt"], "gt", MID, "mean", (0,), Ellipsis)
    assert got.mask[0, 0, 1] and not got.mask[0, 0, 0]
    comp, _ = query(vars_["lt"], "lt", MID, "count", (0,), Ellipsis, components=True)
    assert comp["sum"].data[0, 0, 3] == -np.inf and comp["excess"].data[0, 0, 3] == np.inf


def test_int64_compares_as_float64(gpu):
    """``2**53 + 1`` converts to ``2**53``: not ``gt`` the threshold ``2**53``,
    as documented."""
    for dt in ("<i8", "<u8"):
        x = np.full((6, 2, 8), 2 ** 53 - 1, dt)
        x[1, 0, 0] = 2 ** 53 + 1
        x[2, 0, 0] = 2 ** 53 + 2
        x[3, 0, 1] = 2 ** 53 + 1
        pad = {"gt": 2 ** 60, "ge": 2 ** 60, "lt": 0, "le": 0}
        vars_ = by_op(x, (4, 2, 8), pad=pad)
        thr = float(2 ** 53)
        for axis, path in (((0,), "cols"), ((1,), "walk"), (None, "walk")):
            check_all(x, None, vars_, Ellipsis, axis, thr, path, what=f"{dt} 2^53 {axis}")
        got, _ = query(vars_["gt"], "gt", thr, "count", (0,), Ellipsis)
        assert got.data[0, 0, 0] == 1 and got.data[0, 0, 1] == 0          # 2^53 + 2 alone
        got, _ = query(vars_["ge"], "ge", thr, "count", (0,), Ellipsis)
        assert got.data[0, 0, 0] == 2 and got.data[0, 0, 1] == 1


# -- 7. an empty selection --------------------------------------------------------------------
def test_empty_selection(gpu):
    x, vars_ = walk_var()
    for index, axis, shape in (((slice(4, 4),), (0,), (1, 9, 14)), ((slice(None), slice(5, 5)), (0,), (1, 0, 14)),
                               ((slice(4, 4),), None, (1, 1, 1))):
        for stat in STATS:
            got, took = query(vars_["gt"], "gt", MID, stat, axis, index)
            assert took is None and isinstance(got, np.ma.MaskedArray) and got.shape == shape, (index, stat)
            assert got.dtype == (np.int64 if stat == "count" else np.float64) and got.mask.all(), (index, stat)
        comp, took = query(vars_["gt"], "gt", MID, "count", axis, index, components=True)
        assert took is None and all(v.shape == shape and not (v.data != 0).any() for v in comp.values())


# -- 8. components and exceed.merge -----------------------------------------------------------
def test_components_merge_halves(gpu):
    x = values((36, 6, 20), 81)
    vars_ = by_op(x, (8, 3, 8))
    for thr in (MID, field_for(x.shape, (0,))):
        for op in OPS:
            lo, _ = query(vars_[op], op, thr, "count", (0,), (slice(None, 18),), components=True)
            hi, _ = query(vars_[op], op, thr, "count", (0,), (slice(18, None),), components=True)
            whole, took = query(vars_[op], op, thr, "count", (0,), (slice(None, 36),), components=True)
            assert took == "cols"
            m = exceed.merge(lo, hi)
            o = oracle(x, None, Ellipsis, (0,), op, thr)
            for k in ("n", "n_true"):
                assert np.array_equal(m[k], whole[k].data) and np.array_equal(m[k], o[k]), (op, k)
            for k in ("sum", "excess"):
                bound = sum_bound("float64", o["n_true"], o["abs_" + k])
                assert_within(m[k], o[k], bound, f"merged {op} {k}")
                assert_within(m[k], whole[k].data, 2 * bound, f"merged against whole {op} {k}")
            for stat in STATS:
                check_stat(exceed.finalize(m, stat), o, stat, f"merged {op} {stat}")


# -- 9. determinism, and the two paths against each other -------------------------------------
def test_same_bytes_from_run_to_run_and_equal_counts_on_both_paths(gpu):
    x = values((40, 6, 24), 91)
    var = make_var(x, (8, 3, 8), pad=100)
    field = field_for(x.shape, (0,))
    box = (slice(1, 39), slice(0, 6), slice(2, 23))
    lists = (list(range(1, 39)), list(range(0, 6)), list(range(2, 23)))
    try:
        for thr in (MID, field):
            for stat in ("sum", "excess", "mean"):
                a = Active(var, resident=True)
                first = a.exceed("gt", thr, stat, axis=(0,))[box]
                assert a.exceed_path == "cols"
                again = a.exceed("gt", thr, stat, axis=(0,))[box]
                assert first.data.tobytes() == again.data.tobytes() and np.array_equal(first.mask, again.mask)
                w1 = a.exceed("gt", thr, stat, axis=(0,))[lists]
                assert a.exceed_path == "walk"
                w2 = a.exceed("gt", thr, stat, axis=(0,))[lists]
                assert w1.data.tobytes() == w2.data.tobytes()
            a = Active(var, resident=True)
            a.components = True
            cols = a.exceed("gt", thr, axis=(0,))[box]
            assert a.exceed_path == "cols"
            walk = a.exceed("gt", thr, axis=(0,))[lists]
            assert a.exceed_path == "walk"
            for k in ("n", "n_true"):
                assert np.array_equal(cols[k].data, walk[k].data), k
            o = oracle(x, None, box, (0,), "gt", thr)
            for k in ("sum", "excess"):
                assert_within(cols[k].data, walk[k].data, 2 * sum_bound("float64", o["n_true"], o["abs_" + k]), k)
    finally:
        release_resident(var)


# -- 10. a netCDF file through the HDF5 reader ------------------------------------------------
NC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nc")


def test_netcdf_file(gpu):
    from pyactivestorage_amd.hdf5 import open_variable
    path = os.path.join(NC, "daily_data_masked.nc")
    attrs = open_variable(path, "ta").attrs
    sel = np.ma.asarray(Active(path, "ta")[...])
    data = np.ma.getdata(sel)
    assert np.array_equal(np.ma.getmaskarray(ref.mask_missing(data, get_missing_attributes(attrs))),
                          np.ma.getmaskarray(sel))
    assert np.ma.getmaskarray(sel).any() and not np.ma.getmaskarray(sel).all()
    thr = float(np.ma.median(sel))
    index = tuple(slice(n // 4, n) for n in data.shape)
    for axis in ((0,), None):
        for op in ("gt", "le"):
            o = oracle(data, attrs, index, axis, op, thr)
            a = Active(path, "ta")
            a.components = True
            check_components(a.exceed(op, thr, axis=axis)[index], o, f"file {op} {axis}")
            assert a.exceed_path in ("cols", "walk")
            for stat in STATS:
                a = Active(path, "ta")
                check_stat(a.exceed(op, thr, stat, axis=axis)[index], o, stat, f"file {op} {stat} {axis}")
    assert 0 < oracle(data, attrs, index, None, "gt", thr)["n_true"].item() < data.size


# -- 11. the intended workflow: a percentile field, then the days past it ---------------------
def test_quantile_field_then_fraction(gpu):
    x = np.random.default_rng(111).normal(288.0, 10.0, (60, 5, 12)).astype("<f4")
    var = make_var(x, (16, 3, 8), pad=1000.0)
    a = Active(var)
    t = a.quantile(0.9, axis=(0,))[...]
    assert t.shape == (1, 5, 12)
    want_t = np.quantile(x.astype(np.float64), 0.9, axis=0, keepdims=True)
    np.testing.assert_allclose(np.ma.getdata(t), want_t, rtol=1e-14, atol=0)
    got = a.exceed("gt", t, "fraction", axis=(0,))[...]
    assert a.exceed_path == "cols"
    o = oracle(x, None, Ellipsis, (0,), "gt", want_t)
    check_stat(got, o, "fraction", "TX90p")
    assert np.array_equal(got.data, (x.astype(np.float64) > want_t).sum(axis=0, keepdims=True) / 60.0)
    assert 0.05 < got.mean() < 0.15
    cut = a.exceed("gt", t, "fraction", axis=(0,))[10:50, 1:4, ::3]          # the field follows the global index
    assert a.exceed_path == "walk"
    check_stat(cut, oracle(x, None, (slice(10, 50), slice(1, 4), slice(None, None, 3)), (0,), "gt", want_t),
               "fraction", "TX90p cut")
