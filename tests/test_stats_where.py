"""``Active.argmax`` / ``Active.argmin`` on the device against NumPy.

Oracle: the selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``; per output, by a Python loop, the first
unmasked NaN if there is one, else the first unmasked position equal to the
unmasked maximum / minimum taken in the variable's dtype.  It shares nothing
with ``pyactivestorage_amd/argext.py``.  Every comparison is exact, ``value``
bitwise.  ``argext_path`` is asserted in every case, so a query that silently
took the other kernel fails.

The padding of an edge chunk always beats every real value (above the maximum
for ``argmax``, below the minimum for ``argmin``; where the type leaves no such
value, equal to the extreme), so a kernel that read it would report it.
"""
import functools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import argext
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

WHICH = ("max", "min")
LO, HI = 10, 50                   # the random values' range
PAD = {"max": 100, "min": 1}      # beats every value of the range
TOP, BOTTOM = 60, 5               # planted extremes


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


def _full_index(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    where = [k for k, s in enumerate(index) if s is Ellipsis]
    if where:
        k = where[0]
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def oracle(data, attrs, along, index, which, missing=None):
    """``position`` (in the selection), ``index`` (in the variable), ``value``
    and ``n`` per output, ``along`` kept with extent 1."""
    index = _full_index(index, data.ndim)
    ys = data
    for d, s in enumerate(index):                   # orthogonal: one dim at a time
        ys = ys[(slice(None),) * d + (s,)]
    glob = np.arange(data.shape[along])[index[along]]
    ys = ref.mask_missing(ys, missing or get_missing_attributes(attrs or {}))
    valid = ~np.ma.getmaskarray(ys)
    vals = np.ma.getdata(ys).astype(data.dtype.newbyteorder("="))
    v2 = np.moveaxis(vals, along, 0).reshape(vals.shape[along], -1)
    o2 = np.moveaxis(valid, along, 0).reshape(vals.shape[along], -1)
    n_out = v2.shape[1]
    pos = np.zeros(n_out, dtype=np.int64)
    gidx = np.zeros(n_out, dtype=np.int64)
    val = np.zeros(n_out, dtype=vals.dtype)
    n = np.zeros(n_out, dtype=np.int64)
    for c in range(n_out):
        live = np.nonzero(o2[:, c])[0]
        n[c] = live.size
        if live.size == 0:
            continue
        col = v2[live, c]
        nans = np.nonzero(col != col)[0]
        if nans.size:
            k = live[nans[0]]
        else:
            ext = col.max() if which == "max" else col.min()     # in the variable's dtype
            k = live[np.nonzero(col == ext)[0][0]]
        pos[c], gidx[c], val[c] = k, glob[k], v2[k, c]
    shape = list(vals.shape)
    shape[along] = 1
    return {k: v.reshape(shape) for k, v in (("position", pos), ("index", gidx), ("value", val), ("n", n))}


def query(var, along, which, index, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = (a.argmax if which == "max" else a.argmin)(along)[index]
    return got, a.argext_path


def check_position(got, o, what=""):
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.int64, what
    assert got.shape == o["position"].shape, (what, got.shape, o["position"].shape)
    wm = o["n"] == 0
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    assert np.array_equal(got.data[~wm], o["position"][~wm]), (what, got, o["position"])


def check_components(comp, o, dt, what=""):
    assert sorted(comp) == ["index", "n", "position", "value"], what
    wm = o["n"] == 0
    check_position(comp["position"], o, what)
    assert comp["index"].dtype == np.int64 and np.array_equal(np.ma.getmaskarray(comp["index"]), wm), what
    assert np.array_equal(comp["index"].data[~wm], o["index"][~wm]), (what, "index")
    assert comp["n"].dtype == np.int64 and not np.ma.getmaskarray(comp["n"]).any(), what
    assert np.array_equal(np.ma.getdata(comp["n"]), o["n"]), (what, "n")
    assert comp["value"].dtype == np.dtype(dt).newbyteorder("="), (what, comp["value"].dtype)
    assert np.array_equal(np.ma.getmaskarray(comp["value"]), wm), what
    assert comp["value"].data[~wm].tobytes() == o["value"][~wm].tobytes(), (what, "value")


def check_all(x, attrs, vars_, along, index, path, what="", which=WHICH, missing=None):
    """The plain result and the components of argmax and argmin; ``vars_``:
    the variable per direction (they differ in their padding)."""
    for w in which:
        o = oracle(x, attrs, along, index, w, missing=missing)
        got, took = query(vars_[w], along, w, index)
        assert took == path, (what, w, took)
        check_position(got, o, f"{what} arg{w}")
        comp, took = query(vars_[w], along, w, index, components=True)
        assert took == path, (what, w, took)
        check_components(comp, o, x.dtype, f"{what} arg{w} components")


def both(x, chunks, attrs=None, shuffle=False, pad=None):
    pad = pad or PAD
    return {w: make_var(x, chunks, attrs, shuffle=shuffle, pad=pad[w]) for w in WHICH}


def values(shape, seed, dt="<f4"):
    """Few distinct values: ties in every column."""
    return np.random.default_rng(seed).integers(LO, HI + 1, shape).astype(dt)


# -- 1. the dense column kernel ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layers_var(dt="<f4", chunks=(5, 3, 8), shuffle=False, inner=8):
    """23 rows in layers of 5; the padding of the last layer (rows 23, 24)
    beats every value."""
    x = values((23, 6, inner), 5, dt)
    x[0, 0, 0] = TOP                               # the first row
    x[0, 0, 1] = BOTTOM
    x[22, 0, 2] = TOP                              # the last row
    x[22, 0, 3] = BOTTOM
    x[4, 0, 4] = x[5, 0, 4] = TOP                  # a tie across a layer boundary: row 4
    x[9, 0, 5] = x[10, 0, 5] = BOTTOM
    x[5, 0, 6] = TOP                               # the first row of a layer
    x[14, 0, 7] = BOTTOM                           # the last row of a layer
    x[7, 1, 0] = x[16, 1, 0] = TOP                 # equal extremes in two layers
    x[8, 1, 3] = x[21, 1, 3] = BOTTOM
    x[1, 1, 1] = x[2, 1, 1] = TOP                  # and within the 4 rows in flight
    x[1, 1, 2] = x[3, 1, 2] = BOTTOM
    x[:, 2, 0] = 30                                # a constant column: position 0
    return x, both(x, chunks, shuffle=shuffle)


def test_cols_layers(gpu):
    x, vars_ = layers_var()
    check_all(x, None, vars_, 0, Ellipsis, "cols", what="layers")
    got, _ = query(vars_["max"], 0, "max", Ellipsis)
    assert got.shape == (1, 6, 8)
    assert got.data[0, 0, [0, 2, 4, 6]].tolist() == [0, 22, 4, 5] and got.data[0, 1, :2].tolist() == [7, 1]
    assert got.data[0, 2, 0] == 0
    got, _ = query(vars_["min"], 0, "min", Ellipsis)
    assert got.data[0, 0, [1, 3, 5, 7]].tolist() == [0, 22, 9, 14] and got.data[0, 1, 2:4].tolist() == [1, 8]


def test_cols_box_cuts_items(gpu):
    x, vars_ = layers_var()
    check_all(x, None, vars_, 0, (slice(3, 20), slice(1, None), slice(2, 7)), "cols", what="box")
    check_all(x, None, vars_, 0, (slice(3, 20), slice(0, 4), slice(5, 6)), "cols", what="box of one")   # one output per row
    got, _ = query(vars_["max"], 0, "max", (slice(3, 20), slice(0, 4), slice(4, 5)))
    assert got.data[0, 0, 0] == 1                  # row 4 is position 1 of [3:20]


def test_cols_rows_not_a_multiple_of_4(gpu):
    x, vars_ = layers_var(chunks=(5, 3, 6), inner=11)
    check_all(x, None, vars_, 0, Ellipsis, "cols", what="rows of 6")
    check_all(x, None, vars_, 0, (slice(2, 22), slice(None), slice(1, 10)), "cols", what="rows of 6, box")


@pytest.mark.parametrize("dt", ["<f4", "<f8", "<i2"])
def test_cols_shuffled(gpu, dt):
    x, vars_ = layers_var(dt=dt, shuffle=True)
    check_all(x, None, vars_, 0, Ellipsis, "cols", what=f"shuffled {dt}")
    check_all(x, None, vars_, 0, (slice(3, 20), slice(1, None), slice(2, 7)), "cols", what=f"shuffled {dt} box")


@pytest.mark.parametrize("dt", [">f4", ">i2", ">f8", ">u4"])
def test_cols_big_endian(gpu, dt):
    x, vars_ = layers_var(dt=dt)
    check_all(x, None, vars_, 0, Ellipsis, "cols", what=f"big-endian {dt}")


def test_cols_staging_pass(gpu):
    """1030-row layers: extremes on both sides of the 1024-row staging pass and
    of the layer boundary, and in the very last row."""
    x = values((2070, 2, 8), 9)
    for k, row in enumerate((1023, 1024, 1029, 1030, 2069)):
        x[row, 0, k] = TOP
        x[row, 1, k] = BOTTOM
    x[1023, 0, 5] = x[1024, 0, 5] = TOP            # ties across the pass and across the layer: the first wins
    x[1029, 1, 5] = x[1030, 1, 5] = BOTTOM
    x[0, 0, 6] = x[2069, 0, 6] = TOP               # cut away by [1:2069]: the next best wins
    x[0, 1, 6] = x[2069, 1, 6] = BOTTOM
    vars_ = both(x, (1030, 2, 8))
    check_all(x, None, vars_, 0, Ellipsis, "cols", what="staging")
    check_all(x, None, vars_, 0, (slice(1, 2069),), "cols", what="staging, cut")
    got, _ = query(vars_["max"], 0, "max", Ellipsis)
    assert got.data[0, 0, :6].tolist() == [1023, 1024, 1029, 1030, 2069, 1023]


DTYPES = ["|i1", "|u1", "<i2", "<u2", "<i4", "<u4", "<i8", "<u8", "<f4", "<f8"]


@pytest.mark.parametrize("dt", DTYPES)
def test_cols_dtypes(gpu, dt):
    """int64 near 2^60 and uint64 near 2^63: neighbours that tie only after
    ``astype(float64)``, so a float64 comparison reports an earlier position.
    The type minimum as the argmin winner (i1, i8).  Floats: a NaN after a
    larger value, two NaNs, a NaN in a column whose larger values a valid_max
    rule masks (the NaN itself compares false and stays unmasked: it wins),
    and zeros of both signs in both orders."""
    d = np.dtype(dt)
    rng = np.random.default_rng(20 + DTYPES.index(dt))
    attrs, pad = None, PAD
    if d.itemsize == 8 and d.kind in "iu":
        e = 60 if d.kind == "i" else 63
        vals = np.array([2 ** e - 2, 2 ** e - 1, 2 ** e, 2 ** e + 1, 2 ** e + 2], dtype=d)
        assert len(set(vals.astype(np.float64).tolist())) == 1            # one float64, five integers
        x = vals[rng.integers(0, 5, (23, 6, 8))]
        x[:, 0, 0] = vals[[1, 2, 3, 2, 1, 0, 4, 4, 0] + [2] * 14]          # max at 6, min at 5: float64 says 0
        pad = {"max": 2 ** e + 9, "min": 2 ** e - 9}
        if d.kind == "i":
            x[13, 0, 1] = np.iinfo(d).min
            pad["min"] = np.iinfo(d).min                                   # nothing lies below: the tie must lose
    else:
        x = values((23, 6, 8), 21, d)
        if dt == "|i1":
            x[13, 0, 1] = x[17, 0, 1] = -128
            pad = {"max": 100, "min": -128}
        if d.kind == "f":
            x[3, 0, 0], x[4, 0, 0] = 1e6, np.nan       # a NaN later than a larger value: the NaN
            x[11, 0, 1] = x[6, 0, 1] = np.nan          # two NaNs: the first
            x[2, 0, 2], x[8, 0, 2] = 700.0, np.nan     # the larger value is masked, the NaN is not
            x[20, 0, 3] = 700.0                        # masked: cannot win
            x[:, 1, 0] = 20
            x[5, 1, 0], x[6, 1, 0] = -0.0, 0.0         # argmin: -0.0 first, it wins with its sign
            x[:, 1, 1] = -20
            x[5, 1, 1], x[6, 1, 1] = 0.0, -0.0         # argmax: +0.0 first
            x[:, 1, 2] = 20
            x[5, 1, 2], x[6, 1, 2] = 0.0, -0.0         # argmin: +0.0 first
            x[:, 1, 3] = -20
            x[5, 1, 3], x[6, 1, 3] = -0.0, 0.0         # argmax: -0.0 first
            attrs = {"valid_max": np.array([500.0], d)}
            pad = {"max": 400, "min": -400}
    vars_ = both(x, (5, 3, 8), attrs, pad=pad)
    check_all(x, attrs, vars_, 0, Ellipsis, "cols", what=dt)
    check_all(x, attrs, vars_, 0, (slice(1, 22), slice(0, 6), slice(0, 7)), "cols", what=f"{dt} box")
    if d.itemsize == 8 and d.kind in "iu":
        got, _ = query(vars_["max"], 0, "max", Ellipsis)
        assert got.data[0, 0, 0] == 6 and np.argmax(x[:, 0, 0].astype(np.float64)) == 0
        got, _ = query(vars_["min"], 0, "min", Ellipsis)
        assert got.data[0, 0, 0] == 5 and np.argmin(x[:, 0, 0].astype(np.float64)) == 0
    if dt in ("|i1", "<i8"):
        comp, _ = query(vars_["min"], 0, "min", Ellipsis, components=True)
        assert comp["position"].data[0, 0, 1] == 13 and comp["value"].data[0, 0, 1] == np.iinfo(d).min
    if d.kind == "f":
        for w in WHICH:
            comp, _ = query(vars_[w], 0, w, Ellipsis, components=True)
            assert comp["position"].data[0, 0, :3].tolist() == [4, 6, 8], w
            assert np.isnan(comp["value"].data[0, 0, :3]).all(), w
        comp, _ = query(vars_["min"], 0, "min", Ellipsis, components=True)
        assert comp["position"].data[0, 1, 0] == 5 and np.signbit(comp["value"].data[0, 1, 0])
        assert comp["position"].data[0, 1, 2] == 5 and not np.signbit(comp["value"].data[0, 1, 2])
        comp, _ = query(vars_["max"], 0, "max", Ellipsis, components=True)
        assert comp["position"].data[0, 1, 1] == 5 and not np.signbit(comp["value"].data[0, 1, 1])
        assert comp["position"].data[0, 1, 3] == 5 and np.signbit(comp["value"].data[0, 1, 3])


@functools.lru_cache(maxsize=None)
def masked_var():
    """The would-be winners are masked by each of the rules."""
    x = values((23, 6, 8), 33)
    x[7, 0, 0] = 1000.0                            # _FillValue: the largest value
    x[3, 0, 1] = 500.0                             # above valid_max
    x[12, 0, 2] = 2.0                              # below valid_min: the smallest value
    x[6, 0, 3] = -1000.0                           # missing_value: the smallest value
    x[:, 0, 4] = 1000.0                            # a wholly masked column
    x[:, 0, 5] = 1000.0
    x[10:16, 0, 5] = [30, 40, 40, 20, 20, 30]      # masked but for six rows across a layer boundary
    x[5:11, 1, 0] = 500.0                          # a masked stretch across a layer boundary
    attrs = {"_FillValue": np.array([1000.0], "<f4"), "missing_value": np.array([-1000.0], "<f4"),
             "valid_min": np.array([8.0], "<f4"), "valid_max": np.array([400.0], "<f4")}
    pad = {"max": 300.0, "min": 9.0}               # unmasked, and beats every unmasked value
    return x, attrs, both(x, (5, 3, 8), attrs, pad=pad), pad


def test_cols_mask_rules(gpu):
    x, attrs, vars_, pad = masked_var()
    check_all(x, attrs, vars_, 0, Ellipsis, "cols", what="masked")
    got, _ = query(vars_["max"], 0, "max", Ellipsis)
    assert np.ma.getmaskarray(got)[0, 0, 4] and np.ma.getmaskarray(got).sum() == 1
    assert got.data[0, 0, 0] != 7 and got.data[0, 0, 1] != 3 and got.data[0, 0, 5] == 11
    got, _ = query(vars_["min"], 0, "min", Ellipsis)
    assert got.data[0, 0, 2] != 12 and got.data[0, 0, 3] != 6 and got.data[0, 0, 5] == 13
    comp, _ = query(vars_["max"], 0, "max", Ellipsis, components=True)
    n = np.ma.getdata(comp["n"])
    assert n[0, 0, 0] == 22 and n[0, 0, 4] == 0 and n[0, 0, 5] == 6 and n[0, 1, 0] == 17
    # fill value only (mask mode: equality), and thresholds only (mask mode: range)
    for sub in ({"_FillValue": attrs["_FillValue"]}, {"valid_min": attrs["valid_min"], "valid_max": attrs["valid_max"]}):
        check_all(x, sub, both(x, (5, 3, 8), sub, pad=pad), 0, Ellipsis, "cols", what=f"masked {sorted(sub)}")


def test_components_merge_halves(gpu):
    """``value == x[index]``, and two halves joined equal the whole."""
    x, vars_ = layers_var()
    for w in WHICH:
        whole, _ = query(vars_[w], 0, w, Ellipsis, components=True)
        idx = whole["index"].data
        assert np.array_equal(np.take_along_axis(x, idx, 0), whole["value"].data), w
        assert np.array_equal(whole["index"].data, whole["position"].data)        # the whole axis from 0
        assert not np.shares_memory(whole["index"].data, whole["position"].data)
        lo, p1 = query(vars_[w], 0, w, slice(0, 12), components=True)
        hi, p2 = query(vars_[w], 0, w, slice(12, None), components=True)
        assert p1 == p2 == "cols"
        assert np.array_equal(hi["index"].data, hi["position"].data + 12)
        # by global index (no shift), and by position in each half (the second shifted by the first's length)
        for merged in (argext.merge(lo, hi, which=w),
                       argext.merge({**lo, "index": lo["position"]}, {**hi, "index": hi["position"]}, shift=12, which=w)):
            assert np.array_equal(argext.finalize(merged), whole["position"]), w
            assert np.array_equal(merged["n"], np.ma.getdata(whole["n"])), w
            assert argext.values(merged, x.dtype).tobytes() == whole["value"].data.tobytes(), w
    x, attrs, vars_, _ = masked_var()
    for w in WHICH:
        whole, _ = query(vars_[w], 0, w, Ellipsis, components=True)
        lo, _ = query(vars_[w], 0, w, slice(0, 10), components=True)              # column (0, 5): no unmasked element
        hi, _ = query(vars_[w], 0, w, slice(10, None), components=True)
        assert lo["n"].data[0, 0, 5] == 0 and np.ma.getmaskarray(lo["position"])[0, 0, 5]
        merged = argext.merge(lo, hi, which=w)
        got = argext.finalize(merged)
        assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(whole["index"])), w
        assert np.array_equal(got.filled(0), whole["index"].filled(0)), w
        assert merged.tobytes() == argext.merge(hi, lo, which=w).tobytes()        # commutative


# -- 2. the per-element walk -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_var(chunk):
    x = values((5, 150), 31)
    x[0, 60] = x[0, 134] = TOP                     # a tie that spans lanes, words and chunks of 70
    x[1, 64] = x[1, 128] = BOTTOM                  # the same lane, 64 positions apart
    x[2, 149] = TOP                                # the very last position
    x[3, 0] = BOTTOM
    x[4] = 30                                      # constant: position 0
    return x, both(x, (5, chunk))


@pytest.mark.parametrize("chunk", [150, 70])
def test_walk_innermost(gpu, chunk):
    x, vars_ = row_var(chunk)
    check_all(x, None, vars_, 1, Ellipsis, "walk", what=f"innermost, chunks of {chunk}")
    got, _ = query(vars_["max"], -1, "max", Ellipsis)
    assert got.shape == (5, 1) and got.data[:, 0].tolist()[0:3:2] == [60, 149] and got.data[4, 0] == 0
    got, _ = query(vars_["min"], -1, "min", Ellipsis)
    assert got.data[1, 0] == 64 and got.data[3, 0] == 0


@pytest.mark.parametrize("extent", [1, 63, 64, 65, 130])
def test_walk_innermost_extents(gpu, extent):
    x, vars_ = row_var(150)
    for start in (0, 17):
        index = (slice(None), slice(start, start + extent))
        check_all(x, None, vars_, 1, index, "walk", what=f"extent {extent} from {start}")


@functools.lru_cache(maxsize=None)
def middle_var():
    x = values((5, 23, 7), 41, "<i2")
    x[1, 4, 2] = x[1, 5, 2] = x[1, 19, 2] = TOP    # a tie across chunks of 5 along the middle dim
    x[2, 9, 3] = x[2, 10, 3] = BOTTOM
    return x, both(x, (2, 5, 4))


def test_walk_middle_dim(gpu):
    x, vars_ = middle_var()
    check_all(x, None, vars_, 1, Ellipsis, "walk", what="middle")
    check_all(x, None, vars_, 1, (slice(1, 5), slice(2, 21), slice(1, 6)), "walk", what="middle box")
    check_all(x, None, vars_, 0, Ellipsis, "cols", what="middle var, along 0")
    got, _ = query(vars_["max"], 1, "max", Ellipsis)
    assert got.shape == (5, 1, 7) and got.data[1, 0, 2] == 4


SELECTIONS = [
    ("stride", (slice(1, None, 3),)),
    ("list", ([0, 2, 3, 4, 9, 10, 11, 12, 13, 19, 22],)),
    ("bool", (np.arange(23) % 5 != 2,)),
    ("kept list", (slice(None), [4, 0, 5], slice(None))),
    ("kept lists", ([1, 4, 5, 16, 21], [4, 0, 5], [7, 1])),
    ("kept stride", (slice(None), slice(None), slice(0, None, 2))),
]


@pytest.mark.parametrize("name,index", SELECTIONS, ids=[s[0].replace(" ", "-") for s in SELECTIONS])
def test_walk_selections(gpu, name, index):
    x, vars_ = layers_var()
    check_all(x, None, vars_, 0, index, "walk", what=name)
    x, attrs, vars_, _ = masked_var()
    check_all(x, attrs, vars_, 0, index, "walk", what=f"{name}, masked")


def test_walk_1d_two_fold_levels(gpu):
    """130 chunks of 7: the chunks' records fold in two levels of 64; ties
    span chunks and the level boundary (chunk 64 starts at element 448)."""
    x = values((908,), 51)
    x[440] = x[455] = x[907] = TOP
    x[3] = x[447] = x[448] = BOTTOM
    vars_ = both(x, (7,))
    check_all(x, None, vars_, 0, Ellipsis, "walk", what="1-D")
    check_all(x, None, vars_, 0, (slice(4, 900),), "walk", what="1-D cut")
    check_all(x, None, vars_, 0, (slice(2, None, 2),), "walk", what="1-D stride")
    got, _ = query(vars_["max"], 0, "max", Ellipsis)
    assert got.shape == (1,) and got.data[0] == 440
    got, _ = query(vars_["min"], 0, "min", (slice(4, 900),))
    assert got.data[0] == 443


def test_vector_fill_value_takes_the_walk(gpu):
    x = values((20, 6, 10), 60)                                # whole chunks: vector fill values need equal selections
    vec = np.array([91.0, 92.0, 93.0, 94.0, 95.0], "<f4")        # above every value: would win argmax
    hit = np.random.default_rng(61).random(x.shape) < 0.15
    x[hit] = np.broadcast_to(np.tile(vec, 2), x.shape)[hit]
    x[:, 0, 0] = 91.0                                            # a wholly masked column
    vars_ = both(x, (5, 3, 5), {"_FillValue": vec})
    missing = (np.tile(vec, 2), None, None, None)
    for along in (0, 2):
        check_all(x, None, vars_, along, Ellipsis, "walk", what=f"vector fill along {along}", missing=missing)
    got, _ = query(vars_["max"], 0, "max", Ellipsis)
    assert np.ma.getmaskarray(got)[0, 0, 0]


def test_empty_selection(gpu):
    x, vars_ = layers_var()
    for index, shape in (((slice(4, 4),), (1, 6, 8)), ((slice(None), slice(5, 5)), (1, 0, 8))):
        for w in WHICH:
            a = Active(vars_[w])
            got = (a.argmax if w == "max" else a.argmin)(0)[index]
            assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.int64 and got.shape == shape
            assert np.ma.getmaskarray(got).all() and a.argext_path is None
            a.components = True
            comp = a.argmax(0)[index]
            assert sorted(comp) == ["index", "n", "position", "value"]
            assert comp["position"].shape == shape and comp["n"].shape == shape and comp["n"].dtype == np.int64
            assert comp["value"].dtype == x.dtype and np.ma.getmaskarray(comp["value"]).all()


# -- 3. both paths, run to run ---------------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


def test_both_paths_agree(gpu):
    """``[0:T]`` (the column kernel) against the explicit list ``arange(T)``
    and a full boolean mask (the walk): the same records."""
    xm, attrs, vm, _ = masked_var()
    for (x, vars_) in (layers_var(), (xm, vm)):
        T = x.shape[0]
        for w in WHICH:
            cols, p0 = query(vars_[w], 0, w, (slice(0, T),), components=True)
            assert p0 == "cols"
            for index in ((list(range(T)),), (np.ones(T, dtype=bool),)):
                walk, p1 = query(vars_[w], 0, w, index, components=True)
                assert p1 == "walk"
                for k in cols:
                    assert _bytes(cols[k]) == _bytes(walk[k]), (w, k)


def test_settings_hold_for_one_query(gpu):
    x, vars_ = layers_var()
    a = Active(vars_["max"])
    got = a.argmax(0)[...]
    assert a._method is None and a._argext is None and a.argext_path == "cols"
    check_position(got, oracle(x, None, 0, Ellipsis, "max"), "first")
    mean = a.mean()[...]                                          # the next query is a plain mean over axis 0
    assert mean.shape == (1, 6, 8) and a.argext_path == "cols"
    with pytest.raises(ValueError, match="strictly increasing"):
        a.argmin(0)[[3, 1]]
    assert a._argext is None and a._method is None
