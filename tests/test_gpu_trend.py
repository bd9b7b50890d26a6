"""``Active.trend`` on the device against NumPy.

Oracle: the selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``, converted to float64; ``X`` the
coordinate at the selected global indices, broadcast along ``along``; n, the
means, ``m2_x``, ``m2_y`` and ``cxy`` two-pass over ``axis``
(``keepdims=True``).  For ``axis=None`` the oracle itself is checked against
``np.polyfit`` on centred ``x``.

Tolerance, from the co-moment bound ``TOL = 1e-9`` of
``tests/test_gpu_comoments.py`` (the error of ``cxy`` is bounded relative to
``sqrt(m2_x m2_y)``) and ``|slope| <= sqrt(m2_y / m2_x)``:

    |slope - want|     <= 2e-9 sqrt(m2_y / m2_x)
    |intercept - want| <= |mean_x| (that bound) + 1e-12 (mean|y| + |slope| mean|x|)

A CPU emulation of the lane sums and Chan merges (lanes of 1 to 250 elements
over 1,000 points; coordinates arange, 6e4 + days, 1.7e9 + 86,400 k seconds,
irregular month lengths, fractional years) stayed below 5e-4 of the slope
bound and the float64 oracle below 1e-7 of it, so neither side comes near it.
Masks, ``n`` and NaN positions are exact; the dtype is float64.

Every check prints its largest error as a fraction of the bound.  Largest
over this file, measured on an MI355X: 1.11e-5 of the slope's bound and 7.3e-6
of the intercept's (the dense path's edge cases alone: 8.5e-7).
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import comoments, trend
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

TOL = 1e-9                            # the project's co-moment bound
WORST = {"slope": 0.0, "intercept": 0.0}    # the largest errors seen, as fractions of the bounds above


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


def months(n, start=6e4):
    """An irregular, increasing coordinate: cumulative month lengths from
    ``start`` (under ``arange`` a wrong origin or a constant index offset would
    leave the slope unchanged)."""
    days = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], dtype=np.float64)
    return start + np.concatenate([[0.0], np.cumsum(np.resize(days, n - 1))]) if n > 1 else np.array([start])


def _full_index(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    if Ellipsis in index:
        k = index.index(Ellipsis)
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def _plain(a, fill=0.0):
    return np.where(np.ma.getmaskarray(a), fill, np.ma.getdata(a)).astype(np.float64)


def oracle(data, attrs, coord, along, index, axis, missing=None):
    """n, the means, m2_x, m2_y, cxy, mean|x| and mean|y| of the unmasked selected elements."""
    index = _full_index(index, data.ndim)
    ys = ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {}))
    m = np.ma.getmaskarray(ys)
    y64 = np.ma.MaskedArray(np.ma.getdata(ys).astype(np.float64), mask=m)
    coord = np.arange(data.shape[along], dtype=np.float64) if coord is None else np.asarray(coord, np.float64)
    cx = coord[np.arange(data.shape[along])[index[along]]]        # the selected global indices' coordinates
    shape = [1] * data.ndim
    shape[along] = cx.size
    x64 = np.ma.MaskedArray(np.broadcast_to(cx.reshape(shape), y64.shape), mask=m)
    with np.errstate(all="ignore"):
        n = (~m).sum(axis=axis, keepdims=True)
        div = np.maximum(n, 1)
        mean_x = _plain(x64.sum(axis=axis, keepdims=True)) / div
        mean_y = _plain(y64.sum(axis=axis, keepdims=True)) / div
        dx, dy = x64 - mean_x, y64 - mean_y
        o = {"n": n, "mean_x": mean_x, "mean_y": mean_y,
             "m2_x": _plain((dx * dx).sum(axis=axis, keepdims=True)),
             "m2_y": _plain((dy * dy).sum(axis=axis, keepdims=True)),
             "cxy": _plain((dx * dy).sum(axis=axis, keepdims=True)),
             "abs_x": _plain(np.abs(x64).sum(axis=axis, keepdims=True)) / div,
             "abs_y": _plain(np.abs(y64).sum(axis=axis, keepdims=True)) / div}
        # (np.ma sums skip nothing that is unmasked: a counted NaN or inf reaches m2_y and cxy)
        if axis is None and int(n.reshape(-1)[0]) >= 2:   # the oracle itself against np.polyfit on centred x
            xc, yc = x64.compressed(), y64.compressed()
            if np.isfinite(yc).all() and xc.std() > 0:
                b = np.polyfit(xc - xc.mean(), yc, 1)[0]
                scale = float(np.sqrt(o["m2_y"] / o["m2_x"]).reshape(-1)[0])
                assert abs(float((o["cxy"] / o["m2_x"]).reshape(-1)[0]) - b) <= 1e-10 * scale + 1e-300
    return o


def check(got, o, what="", which="slope"):
    """``got`` (a slope or intercept result) against the oracle's components."""
    assert isinstance(got, np.ma.MaskedArray), what
    n = o["n"]
    assert got.dtype == np.float64 and got.shape == n.shape, (what, got.shape, n.shape)
    with np.errstate(all="ignore"):
        slope = o["cxy"] / o["m2_x"]                               # 0 / 0: NaN
        bound = 2 * TOL * np.sqrt(o["m2_y"] / o["m2_x"])
        want = slope
        if which == "intercept":
            want = o["mean_y"] - slope * o["mean_x"]
            bound = np.abs(o["mean_x"]) * bound + 1e-12 * (o["abs_y"] + np.abs(slope) * o["abs_x"])
    wm = n == 0
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    g, w, b = got.data[~wm], want[~wm], bound[~wm]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, int(np.isnan(g).sum()), int(nan.sum()))
    err = np.abs(g[~nan] - w[~nan])
    bb = b[~nan]
    ok = err <= bb
    frac = float((err[bb > 0] / bb[bb > 0]).max(initial=0.0))
    WORST[which] = max(WORST[which], frac)
    print(what, which, "largest error as a fraction of its bound", frac, "(largest so far", WORST[which], ")")
    assert ok.all(), (what, which, float(err.max()), float(bb[~ok].min()))


def query(var, along, coord, axis, index, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = a.trend(along, coord=coord, axis=axis)[index]
    return got, a.trend_path


def is_prefix(axis, ndim):
    return axis is not None and len(axis) < ndim and tuple(sorted(axis)) == tuple(range(len(axis)))


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
COORDS = [months(n) for n in SHAPE]
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8"]
INDEXES = [
    ("all", (Ellipsis,)),
    ("inner", (slice(1, -1), slice(1, -1), slice(1, -1))),
    ("stride", (slice(None), slice(None, None, 3), slice(None))),
    ("list", (slice(None), [0, 5, 6, 21], slice(None))),
    # [::-2, :, 3:30] as an index list (the planner takes slices of step >= 1 only)
    ("neg", (list(range(14, -1, -2)), slice(None), slice(3, 30))),
]
NUMPY_INDEX = {"neg": (slice(None, None, -2), slice(None), slice(3, 30))}
BOXES = ("all", "inner")


def axes_with(along):
    """Every set of axes that holds ``along``: None (all), (along,), the two pairs."""
    others = [d for d in range(3) if d != along]
    return [None, (along,)] + [tuple(sorted((along, d))) for d in others]


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked, shuffle):
    """Noise about a plane that slopes along every dim.  Masked: 2 % fill
    values with valid_min / valid_max and a few values beyond them."""
    d = np.dtype(dt)
    rng = np.random.default_rng(300 + DTYPES.index(dt))
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    if d.kind == "f":
        x = rng.normal(288.0, 10.0, SHAPE) + 0.8 * i0 - 0.3 * i1 + 0.1 * i2
        fill, lo, hi = -999.0, 200.0, 380.0
    elif d == np.dtype("<i8"):
        x = rng.integers(-2 ** 55, 2 ** 55, SHAPE) * 2 + 1 + 2 ** 50 * i0 - 2 ** 49 * i1
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 60), 2 ** 60
    elif d == np.dtype("|u1"):
        x = rng.integers(10, 200, SHAPE) + 2 * i0 + i1
        fill, lo, hi = 255, 5, 250
    else:
        x = rng.integers(-3000, 3000, SHAPE) + 40 * i0 - 20 * i1 + 7 * i2
        fill, lo, hi = -32768, -4100, 4100
    x = x.astype(d)
    attrs = {}
    if masked:
        f = x.reshape(-1)
        pos = rng.permutation(f.size)
        nf = f.size // 50
        f[pos[:nf]] = fill
        if d.kind == "f" or d == np.dtype("<i2"):
            f[pos[nf:nf + 20]] = d.type(lo - 50)
            f[pos[nf + 20:nf + 40]] = d.type(hi + 50)
        one = lambda v: np.array([v], dtype=d.newbyteorder("="))
        attrs = {"_FillValue": one(fill), "valid_min": one(lo), "valid_max": one(hi)}
    return x, attrs, make_var(x, CHUNKS, attrs, shuffle=shuffle, pad=fill)


def _sweep_cases():
    for dt, (iname, index), masked, shuffle in itertools.product(DTYPES, INDEXES, (False, True), (False, True)):
        if shuffle and np.dtype(dt).itemsize == 1:
            continue   # the byte shuffle of 1-byte elements is the identity: no such layout
        yield pytest.param(dt, iname, index, masked, shuffle,
                           id=f"{dt.replace('|', '=')}-{iname}-{'masked' if masked else 'plain'}-"
                              f"{'shuffled' if shuffle else 'stored'}")


@pytest.mark.parametrize("dt,iname,index,masked,shuffle", list(_sweep_cases()))
def test_sweep(gpu, dt, iname, index, masked, shuffle):
    """Every ``along`` and every set of axes that holds it."""
    x, attrs, var = sweep_var(dt, masked, shuffle)
    for along in range(3):
        for axis in axes_with(along):
            got, path = query(var, along, COORDS[along], axis, index)
            what = f"{dt} {iname} along {along} axis {axis}"
            check(got, oracle(x, attrs, COORDS[along], along, NUMPY_INDEX.get(iname, index), axis), what)
            assert path == ("cols" if iname in BOXES and is_prefix(axis, 3) else "walk"), (what, path)


# -- 2. the dense path's edges ---------------------------------------------------
@pytest.fixture
def low_fill(gpu):
    """The fold's workgroup floor lowered, so that no fill threshold keeps a
    tiny shape from the dense kernel."""
    gpu.set_fold_min_blocks(1)
    yield gpu
    gpu.set_fold_min_blocks(0)


HUGE = 1e30   # planted in the chunks' padding: one element of it in a sum would show in the slope


@functools.lru_cache(maxsize=None)
def edge_var(name):
    rng = np.random.default_rng(77)
    shape, chunks, dt, shuffle, pad = {
        "f4": ((21, 8, 32), (8, 4, 16), "<f4", False, HUGE),
        "i2": ((21, 8, 27), (8, 4, 10), "<i2", False, 32767),
        "u1": ((21, 8, 20), (8, 4, 7), "|u1", False, 255),
        "f8s": ((21, 8, 32), (8, 4, 16), "<f8", True, HUGE),
        "rank2": ((21, 40), (8, 16), "<f4", False, HUGE),
        "rank4": ((5, 9, 6, 20), (2, 4, 3, 8), "<f4", False, HUGE),
        "rank1": ((50,), (16,), "<f4", False, HUGE),
    }[name]
    grids = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    if np.dtype(dt).kind == "f":
        x = rng.normal(288.0, 10.0, shape) + 0.7 * grids[0] - 0.2 * grids[-1]
    elif dt == "|u1":
        x = rng.integers(10, 150, shape) + 3 * grids[0]
    else:
        x = rng.integers(-3000, 3000, shape) + 40 * grids[0] - 9 * grids[-1]
    x = x.astype(dt)
    return x, make_var(x, chunks, shuffle=shuffle, pad=pad)


EDGES = [
    # three chunk layers, the last with 5 valid rows, whole and as a box with
    # misaligned starts and a cut first and last layer
    ("f4", 0, (0,), (Ellipsis,), "cols"),
    ("f4", 0, (0,), (slice(3, 19), slice(1, 7), slice(2, 29)), "cols"),
    ("f4", 1, (0, 1), (slice(3, 19), slice(1, 7), slice(2, 29)), "cols"),
    ("f4", 0, (0,), (slice(3, 19), slice(1, 7), slice(5, 6)), "cols"),      # one output per row
    # rows that are no multiple of 16 bytes
    ("i2", 0, (0,), (Ellipsis,), "cols"),
    ("i2", 0, (0,), (slice(1, 20), slice(None), slice(3, 25)), "cols"),
    ("u1", 0, (0,), (Ellipsis,), "cols"),
    ("u1", 0, (0, 1), (slice(2, None), slice(1, None), slice(1, 19)), "cols"),
    # byte planes
    ("f8s", 0, (0,), (Ellipsis,), "cols"),
    ("f8s", 0, (0,), (slice(3, 19), slice(1, 7), slice(2, 29)), "cols"),
    ("rank2", 0, (0,), (Ellipsis,), "cols"),
    ("rank2", 0, (0,), (slice(2, 20), slice(3, 37)), "cols"),
    ("rank4", 1, (0, 1), (Ellipsis,), "cols"),
    ("rank4", 0, (0, 1), (slice(1, 5), slice(1, 8), slice(None), slice(2, 19)), "cols"),
    ("rank4", 1, (1,), (Ellipsis,), "walk"),                                 # not a prefix
    ("rank4", 2, (0, 1, 2), (Ellipsis,), "cols"),
    ("rank1", 0, (0,), (Ellipsis,), "walk"),                                 # every axis reduced
    ("rank1", 0, None, (slice(3, 47),), "walk"),
]


@pytest.mark.parametrize("name,along,axis,index,path", EDGES,
                         ids=[f"{e[0]}-along{e[1]}-{''.join(map(str, e[2] or ('all',)))}-{k}"
                              for k, e in enumerate(EDGES)])
def test_dense_edges(low_fill, name, along, axis, index, path):
    x, var = edge_var(name)
    coord = months(x.shape[along])
    got, took = query(var, along, coord, axis, index)
    assert took == path
    check(got, oracle(x, None, coord, along, index, axis), f"{name} {index}")
    comp, _ = query(var, along, coord, axis, index, components=True)
    check(comp["intercept"], oracle(x, None, coord, along, index, axis), f"{name} {index}", "intercept")


# -- 3. values ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_var():
    rng = np.random.default_rng(31)
    x = rng.normal(10.0, 3.0, (9, 12, 10)).astype("<f4") + 0.5 * np.arange(9, dtype="<f4")[:, None, None]
    x[:, 7, 3] = -999.0                   # a fully masked column
    x[:, 8, 2] = -999.0                   # a column with one unmasked element
    x[5, 8, 2] = 12.5
    x[:, 9, 2] = -999.0                   # and one with two
    x[2, 9, 2], x[7, 9, 2] = 11.0, 14.5
    x[:, 3, 4] = 287.65                   # constant data
    x[4, 5, 6] = np.nan                   # an unmasked NaN
    x[6, 5, 7] = np.inf
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    return x, attrs, make_var(x, (4, 6, 5), attrs, pad=-999.0)


@pytest.mark.parametrize("index,path", [((Ellipsis,), "cols"), ((slice(None, None, 1), slice(0, 12, 1), [0, 2, 3, 4, 6, 7]),
                                                               "walk")], ids=["cols", "walk"])
def test_values(low_fill, index, path):
    x, attrs, var = value_var()
    coord = months(9)
    a = Active(var)
    a.components = True
    got = a.trend(0, coord=coord, axis=(0,))[index]
    assert a.trend_path == path
    o = oracle(x, attrs, coord, 0, index, (0,))
    check(got["slope"], o, f"values {path}")
    check(got["intercept"], o, f"values {path}", "intercept")
    s, n = got["slope"], np.ma.getdata(got["n"])
    col = {0: 0, 2: 1, 3: 2, 4: 3, 6: 4, 7: 5} if path == "walk" else {k: k for k in range(10)}
    assert np.ma.getmaskarray(s)[0, 7, col[3]] and n[0, 7, col[3]] == 0          # fully masked: masked
    assert n[0, 8, col[2]] == 1 and not np.ma.getmaskarray(s)[0, 8, col[2]] and np.isnan(s.data[0, 8, col[2]])
    assert n[0, 9, col[2]] == 2
    two = (14.5 - 11.0) / (coord[7] - coord[2])                                  # the two-point slope
    assert abs(s.data[0, 9, col[2]] - two) <= 2 * TOL * abs(two)
    assert s.data[0, 3, col[4]] == 0.0 and not np.ma.getmaskarray(s)[0, 3, col[4]]   # constant data: exactly 0
    nan = np.isnan(s.data) & ~np.ma.getmaskarray(s)
    want = np.zeros_like(nan)
    want[0, 8, col[2]] = want[0, 5, col[6]] = want[0, 5, col[7]] = True          # NaN at those outputs only
    assert np.array_equal(nan, want)


def test_equal_coordinates_give_nan(low_fill):
    x, attrs, var = value_var()
    for index, path in (((Ellipsis,), "cols"), ((slice(None), slice(None, None, 2)), "walk")):
        got, took = query(var, 0, np.full(9, 2.5), (0,), index)
        assert took == path
        m = np.ma.getmaskarray(got)
        assert np.isnan(got.data[~m]).all() and m.sum() == (1 if path == "cols" else 0)
        check(got, oracle(x, attrs, np.full(9, 2.5), 0, index, (0,)), f"equal coordinates {path}")


@pytest.mark.parametrize("dt", ["<i2", "<i8", "|u1"])
def test_integer_line_recovers_its_slope(low_fill, dt):
    """Integer data exactly linear in an integer coordinate."""
    coord = np.array([3, 4, 6, 7, 11, 12, 13, 17, 18, 20, 21], dtype=np.float64)
    k = np.arange(6 * 9).reshape(6, 9)
    x = (5 * coord[:, None, None] + k[None] + 2).astype(dt)          # slope 5 along dim 0
    var = make_var(x, (4, 4, 5), pad=1)
    for index, axis, path in (((Ellipsis,), (0,), "cols"), ((slice(1, 10), slice(1, 5), slice(2, 9)), (0,), "cols"),
                              ((Ellipsis,), (0, 2), "walk")):
        got, took = query(var, 0, coord, axis, index)
        assert took == path and not np.ma.getmaskarray(got).any()
        check(got, oracle(x, None, coord, 0, index, axis), f"line {dt} {axis}")
        if axis == (0,):
            assert np.abs(got.data - 5.0).max() <= 2 * TOL * 5.0


@pytest.mark.parametrize("index", [(slice(1, None, 3),), ([0, 2, 3, 9, 13],)], ids=["stride3", "list"])
def test_selection_along_uses_its_global_indices(gpu, index):
    x, attrs, var = sweep_var("<f4", True, False)
    for axis in ((0,), (0, 2), None):
        got, path = query(var, 0, COORDS[0], axis, index)
        assert path == "walk"
        check(got, oracle(x, attrs, COORDS[0], 0, index, axis), f"along selection {index} {axis}")
    # a coordinate that decreases and repeats
    coord = COORDS[0][::-1].copy()
    coord[3] = coord[4]
    got, _ = query(var, 0, coord, (0,), index)
    check(got, oracle(x, attrs, coord, 0, index, (0,)), f"along selection {index}, decreasing coordinate")


# -- 4. other behaviour -------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_vector_fill_value_takes_the_walk(gpu, axis):
    rng = np.random.default_rng(41)
    a = rng.normal(10.0, 3.0, (8, 6, 10)).astype("<f4") + np.arange(10, dtype="<f4")
    vec = np.array([1.0, 2.0, 3.0, 4.0, 5.0], "<f4")
    hit = rng.random(a.shape) < 0.1
    a[hit] = np.broadcast_to(np.tile(vec, 2), a.shape)[hit]
    var = make_var(a, (4, 3, 5), {"_FillValue": vec})
    along = 2 if axis == (2,) else 0
    coord = months(a.shape[along])
    got, path = query(var, along, coord, axis, Ellipsis)
    assert path == "walk"
    # the same rule over the whole selection
    check(got, oracle(a, None, coord, along, Ellipsis, axis, missing=(np.tile(vec, 2), None, None, None)), "vector fill")


def test_zero_size_selection(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    for index, axis, shape in (((slice(0, 15), slice(5, 5), slice(None)), (0,), (1, 0, 37)),
                               ((slice(4, 4),), (0,), (1, 22, 37))):
        a = Active(var)
        got = a.trend(0, coord=COORDS[0], axis=axis)[index]
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64 and got.shape == shape
        assert np.ma.getmaskarray(got).all()
        a.components = True
        comp = a.trend(0, coord=COORDS[0], axis=axis)[index]
        assert comp["slope"].shape == shape and comp["n"].shape == shape and comp["n"].dtype == np.int64


def test_components_merge(low_fill):
    x, attrs, var = sweep_var("<f4", True, False)

    def comps(index, axis=(0,)):
        a = Active(var, axis=axis)
        a.components = True
        return a.trend(0, coord=COORDS[0])[index]

    whole, lo, hi = comps(Ellipsis), comps(slice(0, 8)), comps(slice(8, None))
    names = ["cxy", "intercept", "m2_x", "m2_y", "mean_x", "mean_y", "n", "slope"]
    assert sorted(whole) == names
    assert whole["n"].dtype == np.int64 and not np.ma.getmaskarray(whole["n"]).any()
    for k in names:
        if k != "n":
            assert whole[k].dtype == np.float64 and whole[k].shape == (1, 22, 37)
            assert np.array_equal(np.ma.getmaskarray(whole[k]), np.ma.getdata(whole["n"]) == 0)
    o = oracle(x, attrs, COORDS[0], 0, Ellipsis, (0,))
    np.testing.assert_array_equal(np.ma.getdata(whole["n"]), o["n"])
    np.testing.assert_allclose(_plain(whole["mean_x"]), np.where(o["n"] == 0, 0.0, o["mean_x"]), rtol=1e-12)
    np.testing.assert_allclose(_plain(whole["m2_y"]), o["m2_y"], rtol=TOL)
    check(whole["slope"], o, "whole")
    check(whole["intercept"], o, "whole", "intercept")
    rec = lambda c: comoments.records(np.ma.getdata(c["n"]), *(np.ma.getdata(c[k]) for k in
                                                                ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")))
    merged = comoments.merge(rec(lo), rec(hi))
    np.testing.assert_array_equal(merged["count"], np.ma.getdata(whole["n"]))
    check(trend.slope(merged), o, "merged halves")
    check(trend.intercept(merged), o, "merged halves", "intercept")
    np.testing.assert_array_equal(np.ma.getdata(trend.slope(whole)), np.ma.getdata(whole["slope"]))


def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


@pytest.mark.parametrize("axis,index", [((0,), (slice(1, -1), slice(None), slice(2, 35))),
                                        ((0, 2), (slice(1, -1), slice(None), slice(2, 35))),
                                        (None, (Ellipsis,)),
                                        ((0,), (slice(None), slice(None, None, 2), slice(None)))],
                         ids=["cols", "grid", "all", "stride"])
def test_deterministic_and_resident(low_fill, axis, index):
    x, attrs, var = sweep_var("<f4", True, True)

    def run(resident):
        return Active(var, axis=axis, resident=resident).trend(0, coord=COORDS[0])[index]

    first = run(False)
    assert _bytes(run(False)) == _bytes(first)
    try:
        assert _bytes(run(True)) == _bytes(first)
        assert _bytes(run(True)) == _bytes(first)
    finally:
        release_resident(var)
    assert var._pyas_resident is None


def test_settings_hold_for_one_query(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    a = Active(var, axis=(0,))
    got = a.trend(0, coord=COORDS[0])[...]
    assert a._method is None and a._trend is None and a.trend_path == "cols"
    check(got, oracle(x, attrs, COORDS[0], 0, Ellipsis, (0,)), "first")
    mean = a.mean()[...]                                         # the next query is a plain mean
    assert mean.shape == (1, 22, 37) and a.trend_path == "cols"
    with pytest.raises(ValueError, match="not among the reduced axes"):
        a.trend(1)[...]                                          # the object's axis is still (0,)
    assert a._trend is None
    # coord None: the slope per index step
    got = a.trend(0)[...]
    check(got, oracle(x, attrs, None, 0, Ellipsis, (0,)), "arange")


def teardown_module(module):
    print("test_gpu_trend: largest errors as fractions of the bounds:", WORST)
