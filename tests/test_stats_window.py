"""``Active.rolling`` on the device against NumPy.

Oracle: the selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``, converted with ``astype(float64)``; then a
Python loop over the window starts of every output that adds the window's
elements oldest first and keeps a later sum only when it strictly beats the
holder or is the first NaN.  It shares nothing with
``pyactivestorage_amd/rolling.py``.  Every comparison is exact: values by
equality with NaNs in the same places, positions and counts as integers.
``rolling_path`` is asserted in every case, so a query that silently took the
other kernel fails.
"""
import functools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import rolling
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

COUNTS = ("n_windows", "n", "len")
RAW = ("best", "window", "which", "head", "tail", "head_ok", "tail_ok")


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


def _orthogonal(data, index):
    """``data[index]`` with every list or mask applied to its own dim."""
    for d, s in enumerate(index):
        data = data[(slice(None),) * d + (s,)]
    return data


def oracle(data, attrs, along, index, w, which="max", missing=None):
    """sum, position (-1: no valid window), n_windows, n and len per output
    (``along`` kept with extent 1), by a loop over the window starts."""
    index, along = _full_index(index, data.ndim), along % data.ndim
    ys = ref.mask_missing(_orthogonal(data, index), missing or get_missing_attributes(attrs or {}))
    ok = ~np.ma.getmaskarray(ys)
    x = np.ma.getdata(ys).astype(np.float64)
    T = x.shape[along]
    x2, ok2 = np.moveaxis(x, along, 0).reshape(T, -1), np.moveaxis(ok, along, 0).reshape(T, -1)
    n_out = x2.shape[1]
    o = {"sum": np.zeros(n_out), "position": np.full(n_out, -1, dtype=np.int64),
         "n_windows": np.zeros(n_out, dtype=np.int64), "n": ok2.sum(axis=0).astype(np.int64),
         "len": np.full(n_out, T, dtype=np.int64)}
    with np.errstate(invalid="ignore"):
        for c in range(n_out):
            col, good = x2[:, c].tolist(), ok2[:, c].tolist()
            best, pos, nw = 0.0, -1, 0
            for p in range(T - w + 1):
                if not all(good[p:p + w]):
                    continue
                s = np.float64(col[p])
                for j in range(1, w):
                    s = s + np.float64(col[p + j])
                nw += 1
                if pos < 0:
                    take = True
                elif best != best:
                    take = False
                elif s != s:
                    take = True
                else:
                    take = s < best if which == "min" else s > best
                if take:
                    best, pos = s, p
            o["sum"][c], o["position"][c], o["n_windows"][c] = best, pos, nw
    kept = [s for d, s in enumerate(x.shape) if d != along]
    return {k: np.expand_dims(v.reshape(kept), along) for k, v in o.items()}


def query(var, along, w, index, stat="sum", which="max", components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = a.rolling(along, w, stat=stat, extreme=which)[index]
    return got, a.rolling_path


def check_value(got, o, w, stat="sum", what=""):
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64, what
    assert got.shape == o["sum"].shape, (what, got.shape, o["sum"].shape)
    wm = o["n_windows"] == 0
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    want = o["sum"] / np.float64(w) if stat == "mean" else o["sum"]
    assert np.array_equal(got.data[~wm], want[~wm], equal_nan=True), (what, stat)


def check_components(comp, o, w, which, stat="sum", what=""):
    assert sorted(comp) == sorted(("value", "sum", "position") + COUNTS + RAW), what
    check_value(comp["value"], o, w, stat, what)
    check_value(comp["sum"], o, w, "sum", what)
    wm = o["n_windows"] == 0
    pos = comp["position"]
    assert pos.dtype == np.int64 and np.array_equal(np.ma.getmaskarray(pos), wm), what
    assert np.array_equal(pos.data[~wm], o["position"][~wm]), what
    for k in COUNTS:
        assert comp[k].dtype == np.int64 and not np.ma.getmaskarray(comp[k]).any(), (what, k)
        assert np.array_equal(np.ma.getdata(comp[k]), o[k]), (what, k)
    assert (comp["window"] == w).all() and (comp["which"] == int(which == "min")).all(), what
    assert comp["head"].shape == o["sum"].shape + (7,) and comp["tail"].shape == o["sum"].shape + (7,)


def check_all(x, attrs, var, along, index, path, ws=(5,), whichs=("max",), what="", missing=None):
    """The value for every window and extreme, and the components for the first."""
    for w in ws:
        for which in whichs:
            o = oracle(x, attrs, along, index, w, which, missing)
            got, took = query(var, along, w, index, which=which)
            assert took == path, (what, took)
            check_value(got, o, w, what=f"{what} w={w} {which}")
    comp, took = query(var, along, ws[0], index, which=whichs[0], components=True)
    assert took == path
    check_components(comp, oracle(x, attrs, along, index, ws[0], whichs[0], missing), ws[0], whichs[0], what=what)


def field(shape, seed, dt="<f4", lo=0, hi=9):
    """Small integers: sums are exact, ties are common."""
    return np.random.default_rng(seed).integers(lo, hi, shape).astype(dt)


# -- 1. the dense column kernel ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layers_var(dt="<f4", chunks=(5, 3, 8), shuffle=False, inner=8):
    """23 rows in layers of 5: a window of 5 or 8 spans up to three layers; the
    padding of the last layer (rows 23, 24) holds values that would win."""
    x = field((23, 6, inner), 5, dt)
    x[:, 0, 0] = 1
    x[[3, 4, 5, 6, 7], 0, 0] = 8                   # the best window of 5 lies across layers 0 and 1
    x[:, 0, 1] = 2
    x[18:23, 0, 1] = 7                             # the best one is the last
    x[:, 0, 2] = 3                                 # all equal: the first window wins
    x[:, 0, 3] = 1
    x[[2, 3, 12, 13], 0, 3] = 6                    # equal maxima at two positions
    return x, make_var(x, chunks, shuffle=shuffle, pad=100)


def test_cols_layers(gpu):
    x, var = layers_var()
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5, 8, 1, 2, 3, 4, 6, 7), whichs=("max", "min"), what="layers")
    got, _ = query(var, 0, 5, Ellipsis)
    assert got.shape == (1, 6, 8) and got.data[0, 0, :3].tolist() == [40.0, 35.0, 15.0]
    comp, _ = query(var, 0, 5, Ellipsis, components=True)
    assert comp["position"].data[0, 0, :3].tolist() == [3, 18, 0]
    comp, _ = query(var, 0, 2, Ellipsis, components=True)
    assert comp["position"].data[0, 0, 3] == 2 and comp["sum"].data[0, 0, 3] == 12.0


def test_cols_box_cuts_items(gpu):
    x, var = layers_var()
    index = (slice(3, 20), slice(1, None), slice(2, 7))
    check_all(x, None, var, 0, index, "cols", ws=(5, 8), what="box")
    index = (slice(3, 20), slice(0, 4), slice(5, 6))           # one output per row
    check_all(x, None, var, 0, index, "cols", ws=(3,), what="box of one")


def test_cols_rows_not_a_multiple_of_4(gpu):
    x, var = layers_var(chunks=(5, 3, 6), inner=11)
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5, 8), what="rows of 6")
    check_all(x, None, var, 0, (slice(2, 22), slice(None), slice(1, 10)), "cols", ws=(3,), what="rows of 6, box")


def test_cols_staging_pass(gpu):
    """One chunk of 1030 rows: windows cross the 1024-row staging pass; the
    best ones lie on the seam."""
    x = field((1030, 1, 4), 9)
    x[1020:1028, 0, 0] = 50                        # rows 1020 .. 1027: the seam inside the best window of 8
    x[1023:1025, 0, 1] = 60
    x[1024:1030, 0, 2] = 40                        # begins with the second pass, ends with the chunk
    var = make_var(x, (1030, 1, 4), pad=100)
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(8, 5, 2), what="staging")
    check_all(x, None, var, 0, (slice(1, 1029),), "cols", ws=(5,), what="staging, cut")
    comp, _ = query(var, 0, 8, Ellipsis, components=True)
    assert comp["position"].data[0, 0, 0] == 1020 and comp["sum"].data[0, 0, 0] == 400.0


@pytest.mark.parametrize("dt", ["<f4", "<f8", "<i2"])
def test_cols_shuffled(gpu, dt):
    x, var = layers_var(dt=dt, shuffle=True)
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5,), what=f"shuffled {dt}")
    check_all(x, None, var, 0, (slice(3, 20), slice(1, None), slice(2, 7)), "cols", ws=(8,), what=f"shuffled {dt} box")


@pytest.mark.parametrize("dt", [">f4", ">i2", ">f8", ">u4"])
def test_cols_big_endian(gpu, dt):
    x, var = layers_var(dt=dt)
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5,), whichs=("min",), what=f"big-endian {dt}")


DTYPES = ["|i1", "|u1", "<i2", "<u2", "<i4", "<u4", "<i8", "<u8", "<f4", "<f8"]


@pytest.mark.parametrize("dt", DTYPES)
def test_cols_dtypes(gpu, dt):
    """int64 / uint64: values near 2^60 that ``astype(float64)`` rounds, so the
    sum of the converted elements differs from the converted integer sum."""
    d = np.dtype(dt)
    rng = np.random.default_rng(20 + DTYPES.index(dt))
    if d.itemsize == 8 and d.kind in "iu":
        vals = np.array([2 ** 60 - 1, 2 ** 60 + 1, 2 ** 60 + 129, 2 ** 60 - 2 ** 8, 3, 2 ** 59 + 65], dtype=d)
        x = vals[rng.integers(0, len(vals), (23, 6, 8))]
        x[:2, 0, 0] = vals[[0, 2]]                                                # 2^60 + (2^60 + 256), not 2^61 + 128
        assert np.float64(x[0, 0, 0]) + np.float64(x[1, 0, 0]) == 2.0 ** 61 + 256.0
    elif d.kind == "f":
        x = (rng.integers(-40, 40, (23, 6, 8)) / 8).astype(d) + d.type(0.1)     # inexact sums: the order shows
    else:
        info = np.iinfo(d)
        x = rng.integers(max(info.min, -1000), min(info.max, 1000) + 1, (23, 6, 8)).astype(d)
    var = make_var(x, (5, 3, 8), pad=np.max(x))
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5, 2), whichs=("max", "min"), what=dt)
    check_all(x, None, var, 0, (slice(1, 22), slice(1, 6), slice(1, 7)), "cols", ws=(8,), what=f"{dt} box")


@functools.lru_cache(maxsize=None)
def masked_var():
    """Small integers between the thresholds; each mask rule removes windows."""
    x = field((23, 6, 8), 31, lo=30, hi=40)
    x[7, 0, 0] = 1000.0                            # _FillValue
    x[3, 0, 1] = 500.0                             # above valid_max
    x[12, 0, 2] = 22.0                             # below valid_min
    x[9, 0, 3] = np.nan                            # data, not a missing day
    x[:, 0, 4] = 1000.0                            # a wholly masked column
    x[:, 0, 5] = 1000.0
    x[10:14, 0, 5] = 35.0                          # 4 unmasked positions: no window of 5
    x[:, 0, 6] = 1000.0
    x[10:15, 0, 6] = 35.0                          # exactly 5: one window
    x[5:11, 1, 0] = 500.0                          # a masked stretch across a layer boundary
    x[::4, 1, 1] = 1000.0                          # a masked element in every window of 5
    attrs = {"_FillValue": np.array([1000.0], "<f4"), "valid_min": np.array([25.0], "<f4"),
             "valid_max": np.array([400.0], "<f4")}
    return x, attrs, make_var(x, (5, 3, 8), attrs, pad=399.0)


def test_cols_mask_rules_remove_windows(gpu):
    x, attrs, var = masked_var()
    check_all(x, attrs, var, 0, Ellipsis, "cols", ws=(5, 8, 1), whichs=("max", "min"), what="masked")
    comp, _ = query(var, 0, 5, Ellipsis, components=True)
    nw, n = comp["n_windows"].data, comp["n"].data
    assert nw[0, 2, 2] == 19                                               # 23 - 5 + 1 with nothing masked
    assert nw[0, 0, 0] == nw[0, 0, 2] == 14 and nw[0, 0, 1] == 15          # one masked element removes w windows (4 at row 3)
    assert nw[0, 0, 3] == 19 and n[0, 0, 3] == 23 and np.isnan(comp["value"].data[0, 0, 3])
    assert nw[0, 0, 4] == 0 and n[0, 0, 4] == 0 and nw[0, 0, 5] == 0 and n[0, 0, 5] == 4
    assert nw[0, 0, 6] == 1 and comp["position"].data[0, 0, 6] == 10 and comp["sum"].data[0, 0, 6] == 175.0
    assert nw[0, 1, 1] == 0 and n[0, 1, 1] == 17
    bad = np.ma.getmaskarray(comp["value"])
    assert bad[0, 0, 4] and bad[0, 0, 5] and bad[0, 1, 1] and bad.sum() == 3
    # fill value only (mask mode: equality), and thresholds only (mask mode: range)
    for sub in ({"_FillValue": attrs["_FillValue"]}, {"valid_min": attrs["valid_min"], "valid_max": attrs["valid_max"]}):
        v = make_var(x, (5, 3, 8), sub, pad=399.0)
        check_all(x, sub, v, 0, Ellipsis, "cols", ws=(5,), what=f"masked {sorted(sub)}")


def test_cols_nan_and_infinities(gpu):
    x = field((23, 3, 8), 41)
    x[6, 0, 0] = np.nan                            # the first NaN sum wins, for max and for min
    x[15, 0, 0] = np.nan
    x[4, 0, 1], x[7, 0, 1] = np.inf, -np.inf       # together in a window of 5: a NaN sum; alone: +-inf
    x[4, 0, 2] = np.inf
    x[20, 0, 3] = -np.inf
    x[:, 0, 4] = -0.0
    x[5, 0, 4] = 0.0                               # -0.0 == +0.0: the first window stays
    var = make_var(x, (5, 3, 8), pad=np.inf)
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(5, 3, 1), whichs=("max", "min"), what="nan")
    for which in ("max", "min"):
        comp, _ = query(var, 0, 5, Ellipsis, which=which, components=True)
        assert np.isnan(comp["sum"].data[0, 0, 0]) and comp["position"].data[0, 0, 0] == 2
        assert np.isnan(comp["sum"].data[0, 0, 1]) and comp["position"].data[0, 0, 1] == 3
        assert comp["position"].data[0, 0, 4] == 0
    comp, _ = query(var, 0, 3, Ellipsis, components=True)
    assert comp["sum"].data[0, 0, 1] == np.inf and comp["position"].data[0, 0, 1] == 2


def test_window_of_one_is_max(gpu):
    x, attrs, var = masked_var()
    x = x.copy()
    x[9, 0, 3] = 33.0                              # (np.max would propagate the NaN just the same)
    var = make_var(x, (5, 3, 8), attrs, pad=399.0)
    ys = ref.mask_missing(x, get_missing_attributes(attrs))
    for which, fn in (("max", np.ma.max), ("min", np.ma.min)):
        got, took = query(var, 0, 1, Ellipsis, which=which)
        want = fn(ys, axis=0, keepdims=True)
        assert took == "cols" and np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))
        assert np.array_equal(got.compressed(), want.compressed().astype(np.float64))


def test_mean(gpu):
    x = (field((23, 6, 8), 51) / 8 + 0.1).astype("<f4")
    var = make_var(x, (5, 3, 8), pad=100)
    for w in (3, 5, 7):
        o = oracle(x, None, 0, Ellipsis, w)
        got, took = query(var, 0, w, Ellipsis, stat="mean")
        assert took == "cols"
        check_value(got, o, w, "mean", f"mean w={w}")
    comp, _ = query(var, 0, 3, Ellipsis, stat="mean", which="min", components=True)
    check_components(comp, oracle(x, None, 0, Ellipsis, 3, "min"), 3, "min", "mean", "mean components")


def test_components_merge_halves(gpu):
    """Two halves joined with rolling.merge equal the whole query; in column
    (0, 0) the winning window of 5 lies across the join at row 5."""
    x, var = layers_var()
    for w in (5, 8, 1):
        whole, _ = query(var, 0, w, Ellipsis, components=True)
        lo, p1 = query(var, 0, w, slice(0, 5), components=True)
        hi, p2 = query(var, 0, w, slice(5, None), components=True)
        assert p1 == p2 == "cols"
        merged = rolling.merge(lo, hi)
        for k in rolling.FIELDS:
            assert np.array_equal(merged[k], np.ma.getdata(whole[k])), (w, k)
        for stat in ("sum", "mean"):
            assert np.array_equal(rolling.finalize(merged, stat), rolling.finalize(whole, stat)), (w, stat)
        assert np.array_equal(rolling.finalize(merged), whole["value"])
        if w == 5:
            assert merged["position"][0, 0, 0] == 3 and merged["best"][0, 0, 0] == 40.0
            assert lo["n_windows"].data[0, 0, 0] == 1 and hi["position"].data[0, 0, 0] == 0


# -- 2. the per-element walk -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def middle_var():
    x = field((5, 23, 7), 61, "<i2", -9, 9)
    return x, make_var(x, (2, 5, 4), pad=100)


def test_walk_middle_and_innermost(gpu):
    x, var = middle_var()
    check_all(x, None, var, 1, Ellipsis, "walk", ws=(5, 8), whichs=("max", "min"), what="middle")
    check_all(x, None, var, 1, (slice(1, 5), slice(2, 21), slice(1, 6)), "walk", ws=(3,), what="middle box")
    check_all(x, None, var, 2, Ellipsis, "walk", ws=(5, 2), what="innermost")
    check_all(x, None, var, -1, (slice(None), slice(3, 9), slice(1, 7)), "walk", ws=(3,), what="innermost box")
    check_all(x, None, var, 0, Ellipsis, "cols", ws=(2,), what="middle var, along 0")
    got, _ = query(var, 2, 8, Ellipsis)                        # 7 positions: no window of 8
    assert got.shape == (5, 23, 1) and np.ma.getmaskarray(got).all()


SELECTIONS = [
    ("stride", (slice(1, None, 3),)),
    ("list", ([0, 2, 3, 4, 9, 10, 11, 12, 13, 19, 22],)),
    ("bool", (np.arange(23) % 5 != 2,)),
    ("kept list", (slice(None), [4, 0, 5], slice(None))),
    ("kept stride", (slice(2, 21), slice(None), slice(0, None, 2))),
]


@pytest.mark.parametrize("name,index", SELECTIONS, ids=[s[0].replace(" ", "-") for s in SELECTIONS])
def test_walk_selections(gpu, name, index):
    x, var = layers_var()
    check_all(x, None, var, 0, index, "walk", ws=(5, 3), what=name)
    x, attrs, var = masked_var()
    check_all(x, attrs, var, 0, index, "walk", ws=(3,), whichs=("min",), what=f"{name}, masked")


def test_walk_1d_two_fold_levels(gpu):
    """130 chunks of 3 with a window of 8: every record is shorter than w - 1,
    the chunks' records fold in two levels of 64, and three records merge
    before any window exists."""
    x = field((389,), 71)
    x[188:196] = 9                                 # the best window lies across the level boundary (chunk 64: element 192)
    var = make_var(x, (3,), pad=100)
    check_all(x, None, var, 0, Ellipsis, "walk", ws=(8, 5, 1), whichs=("max", "min"), what="1-D")
    check_all(x, None, var, 0, (slice(4, 380),), "walk", ws=(8,), what="1-D cut")
    check_all(x, None, var, 0, (slice(2, None, 2),), "walk", ws=(8,), what="1-D stride")
    comp, _ = query(var, 0, 8, Ellipsis, components=True)
    assert comp["value"].shape == (1,) and comp["position"].data[0] == 188 and comp["sum"].data[0] == 72.0


def test_vector_fill_value_takes_the_walk(gpu):
    x = field((20, 6, 10), 81, lo=30, hi=36)                     # whole chunks: vector fill values need equal selections
    vec = np.array([31.0, 32.0, 33.0, 34.0, 35.0], "<f4")
    var = make_var(x, (5, 3, 5), {"_FillValue": vec}, pad=100)
    missing = (np.tile(vec, 2), None, None, None)
    for along in (0, 2):
        o = oracle(x, None, along, Ellipsis, 3, missing=missing)
        got, took = query(var, along, 3, Ellipsis)
        assert took == "walk"
        check_value(got, o, 3, what=f"vector fill along {along}")


def test_empty_selection(gpu):
    x, var = layers_var()
    for index, shape in (((slice(4, 4),), (1, 6, 8)), ((slice(None), slice(5, 5)), (1, 0, 8))):
        a = Active(var)
        got = a.rolling(0, 5)[index]
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64 and got.shape == shape
        assert np.ma.getmaskarray(got).all() and a.rolling_path is None
        a.components = True
        comp = a.rolling(0, 5, stat="mean")[index]
        assert comp["value"].shape == shape and comp["n"].shape == shape and comp["n"].dtype == np.int64
        assert comp["head"].shape == shape + (7,)


# -- 3. both paths, run to run ---------------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


def inexact_var():
    x = (field((23, 6, 8), 91) / 8 + 0.1).astype("<f4")
    x[5, 0, 0] = np.nan
    return x, None, make_var(x, (5, 3, 8), pad=100)


def test_both_paths_agree(gpu):
    """``[0:T]`` (the column kernel) against the explicit list ``arange(T)``
    and a full boolean mask (the walk and the combine): the same bytes."""
    for (x, attrs, var) in (inexact_var(), masked_var()):
        T = x.shape[0]
        for w, which in ((5, "max"), (8, "min")):
            cols, p0 = query(var, 0, w, (slice(0, T),), which=which, components=True)
            vals, _ = query(var, 0, w, (slice(0, T),), stat="mean", which=which)
            assert p0 == "cols"
            for index in ((list(range(T)),), (np.ones(T, dtype=bool),)):
                walk, p1 = query(var, 0, w, index, which=which, components=True)
                assert p1 == "walk"
                for k in cols:
                    assert _bytes(cols[k]) == _bytes(walk[k]), (w, k)
                again, p2 = query(var, 0, w, index, stat="mean", which=which)
                assert p2 == "walk" and _bytes(again) == _bytes(vals)


@pytest.mark.parametrize("index,path", [((Ellipsis,), "cols"), ((slice(1, None, 2),), "walk")], ids=["cols", "walk"])
def test_deterministic(gpu, index, path):
    x, attrs, var = inexact_var()
    first, took = query(var, 0, 5, index, components=True)
    assert took == path
    for _ in range(2):
        again, _ = query(var, 0, 5, index, components=True)
        for k in first:
            assert _bytes(again[k]) == _bytes(first[k]), k


def test_settings_hold_for_one_query(gpu):
    x, var = layers_var()
    a = Active(var)
    got = a.rolling(0, 5, stat="mean", extreme="min")[...]
    assert a._method is None and a._rolling is None and a.rolling_path == "cols"
    check_value(got, oracle(x, None, 0, Ellipsis, 5, "min"), 5, "mean", "first")
    mean = a.mean()[...]                                          # the next query is a plain mean over axis 0
    assert mean.shape == (1, 6, 8) and a.rolling_path == "cols"
    with pytest.raises(ValueError, match="strictly increasing"):
        a.rolling(0, 5)[[3, 1]]
    assert a._rolling is None and a._method is None
