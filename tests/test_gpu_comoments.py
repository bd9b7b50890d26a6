"""``Active.cov`` / ``Active.corr`` on the device against NumPy.

Oracle: ``x[index]`` and ``y[index]`` taken with NumPy, each masked with
``oracle.storage_ref.mask_missing`` under its own attributes, the common mask
their OR, both converted to float64; n, the means, ``m2_x``, ``m2_y`` and
``cxy`` with ``np.ma`` over ``axis`` (``keepdims=True``).  For ``axis=None``
the oracle itself is checked against ``np.cov`` / ``np.corrcoef``.

Tolerance (the argument of DESIGN 6.7 for ``var``, carried to the cross
term): a lane's ``sum dx dy`` is off by at most about
``n_lane 2^-53 sum |dx dy|``, and ``sum |dx dy| <= sqrt(m2_x m2_y)`` by
Cauchy-Schwarz, with the same amplification ``1 + (K - mu)^2 / sigma^2`` of the
shift correction.  So the error of ``cxy`` is bounded relative to
``sqrt(m2_x m2_y)``, not to ``cxy`` (which may cancel to 0):

    |cov - want|  <= 1e-9 sqrt(m2_x m2_y) / (n - ddof)
    |corr - want| <= 1e-9

Mask, count and NaN positions are exact; the dtype is float64.
"""
import ctypes
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import _lib, comoments, engine
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

TOL = 1e-9
WORST = {"cov": 0.0, "corr": 0.0}    # the largest errors seen, in units of the bounds above


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


def oracle(x, y, attrs_x, attrs_y, index, axis, missing_x=None, missing_y=None):
    """n, the means, m2_x, m2_y and cxy of the pairs unmasked on both sides."""
    xs = ref.mask_missing(x[index], missing_x or get_missing_attributes(attrs_x or {}))
    ys = ref.mask_missing(y[index], missing_y or get_missing_attributes(attrs_y or {}))
    m = np.ma.getmaskarray(xs) | np.ma.getmaskarray(ys)
    x64 = np.ma.MaskedArray(np.ma.getdata(xs).astype(np.float64), mask=m)
    y64 = np.ma.MaskedArray(np.ma.getdata(ys).astype(np.float64), mask=m)
    with np.errstate(all="ignore"):
        n = (~m).sum(axis=axis, keepdims=True)
        # (np.ma's own mean masks a NaN or infinite quotient: the sums are np.ma's, the division is plain)
        mean_x = _plain(x64.sum(axis=axis, keepdims=True)) / np.maximum(n, 1)
        mean_y = _plain(y64.sum(axis=axis, keepdims=True)) / np.maximum(n, 1)
        dx, dy = x64 - mean_x, y64 - mean_y
        o = {"n": n, "mean_x": np.ma.MaskedArray(mean_x, mask=n == 0),
             "mean_y": np.ma.MaskedArray(mean_y, mask=n == 0),
             "m2_x": (dx * dx).sum(axis=axis, keepdims=True), "m2_y": (dy * dy).sum(axis=axis, keepdims=True),
             "cxy": (dx * dy).sum(axis=axis, keepdims=True)}
        if axis is None and int(n.reshape(-1)[0]) >= 2:   # the oracle itself against np.cov / np.corrcoef
            xc, yc = x64.compressed(), y64.compressed()
            if np.isfinite(xc).all() and np.isfinite(yc).all() and xc.std() > 0 and yc.std() > 0:
                cxy, m2 = float(o["cxy"].reshape(-1)[0]), float(np.sqrt(o["m2_x"] * o["m2_y"]).reshape(-1)[0])
                for ddof in (0, 1):
                    dof = xc.size - ddof
                    assert abs(cxy / dof - np.cov(xc, yc, ddof=ddof)[0, 1]) <= 1e-12 * m2 / dof
                assert abs(cxy / m2 - np.corrcoef(xc, yc)[0, 1]) <= 1e-12
    return o


def _plain(a, fill=0.0):
    return np.where(np.ma.getmaskarray(a), fill, np.ma.getdata(a)).astype(np.float64)


def check(got, o, method, ddof=0, what=""):
    """``got`` (a cov or corr result) against the oracle's components."""
    assert isinstance(got, np.ma.MaskedArray), what
    n = o["n"]
    assert got.dtype == np.float64 and got.shape == n.shape, (what, got.shape, n.shape)
    cxy, m2 = _plain(o["cxy"]), np.sqrt(_plain(o["m2_x"]) * _plain(o["m2_y"]))
    with np.errstate(all="ignore"):
        if method == "cov":
            wm = n - ddof <= 0
            dof = np.where(wm, 1, n - ddof).astype(np.float64)
            want, bound = cxy / dof, TOL * m2 / dof
        else:
            wm = n == 0
            want = np.clip(cxy / np.sqrt(_plain(o["m2_x"])) / np.sqrt(_plain(o["m2_y"])), -1.0, 1.0)
            bound = np.full(n.shape, TOL)
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    g, w, b = got.data[~wm], want[~wm], bound[~wm]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, np.isnan(g).sum(), nan.sum())
    err = np.abs(g[~nan] - w[~nan])
    ok = err <= b[~nan]
    rel = float((err / np.where(b[~nan] > 0, b[~nan], 1.0))[b[~nan] > 0].max(initial=0.0)) * TOL
    WORST[method] = max(WORST[method], rel)
    print(what, method, "largest error over its scale", rel, "(largest so far", WORST[method], ")")
    assert ok.all(), (what, method, float(err.max()), float(b[~nan][~ok].min()))


def query(vx, vy, method, axis, ddof, index, same=False, **kw):
    a = Active(vx, **kw)
    b = a if same else Active(vy, **kw)
    if method == "cov":
        a.cov(b, axis=axis, ddof=ddof)
    else:
        a.corr(b, axis=axis)
    return a[index]


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
PAIRS = [("<f4", "<f4"), ("<f4", ">f4"), ("<f8", "<f8"), ("<i2", "<i2"), ("|u1", "|u1"), ("<i8", "<i8")]
INDEXES = [
    ("all", (Ellipsis,)),
    ("inner", (slice(1, -1), slice(1, -1), slice(1, -1))),
    ("stride", (slice(None), slice(None, None, 3), slice(None))),
    ("list", (slice(None), [0, 5, 6, 21], slice(None))),
    # [::-2, :, 3:30] as an index list (the planner takes slices of step >= 1 only)
    ("neg", (list(range(14, -1, -2)), slice(None), slice(3, 30))),
]
NUMPY_INDEX = {"neg": (slice(None, None, -2), slice(None), slice(3, 30))}
AXES = [None, (0,), (1,), (2,), (0, 2)]
METHODS = [("cov", 0), ("cov", 1), ("corr", 0)]


@functools.lru_cache(maxsize=None)
def sweep_vars(dtx, dty, masked):
    """x as the moments sweep draws it, y = 0.3 x + noise (r about 0.5).  Masked:
    2 % fill in x with valid_min / valid_max, 3 % fill in y at other positions."""
    dx, dy = np.dtype(dtx), np.dtype(dty)
    rng = np.random.default_rng(200 + PAIRS.index((dtx, dty)))
    if dx.kind == "f":
        x = rng.normal(288.0, 10.0, SHAPE)
        y = 0.3 * x + rng.normal(0.0, 5.2, SHAPE)
        fill, lo, hi = -999.0, 200.0, 380.0
    elif dx == np.dtype("<i8"):
        # odd values up to 2^56 in magnitude, spread about zero (see the moments sweep)
        x = rng.integers(-2 ** 55, 2 ** 55, SHAPE) * 2 + 1
        y = (0.3 * x + rng.normal(0.0, 0.52 * 2 ** 55, SHAPE)).astype(np.int64)
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 60), 2 ** 60
    elif dx == np.dtype("|u1"):
        x = rng.integers(10, 240, SHAPE)
        y = np.clip(np.rint(0.3 * x + rng.normal(60.0, 20.0, SHAPE)), 1, 250)
        fill, lo, hi = 255, 5, 250
    else:
        x = rng.integers(-3000, 3000, SHAPE)
        y = np.rint(0.3 * x + rng.normal(0.0, 900.0, SHAPE))
        fill, lo, hi = -32768, -3100, 3100
    x, y = x.astype(dx), y.astype(dy)
    ax, ay = {}, {}
    if masked:
        fx, fy = x.reshape(-1), y.reshape(-1)
        pos = rng.permutation(fx.size)
        nx, ny = fx.size // 50, 3 * fx.size // 100
        fx[pos[:nx]] = fill                         # 2 % in x
        fy[pos[nx:nx + ny]] = fill                  # 3 % in y, elsewhere
        if dx.kind == "f" or dx == np.dtype("<i2"):   # a few beyond valid_min / valid_max, in x only
            fx[pos[nx + ny:nx + ny + 20]] = dx.type(lo - 50)
            fx[pos[nx + ny + 20:nx + ny + 40]] = dx.type(hi + 50)
        one = lambda v, dt: np.array([v], dtype=dt.newbyteorder("="))
        ax = {"_FillValue": one(fill, dx), "valid_min": one(lo, dx), "valid_max": one(hi, dx)}
        ay = {"_FillValue": one(fill, dy)}
    return x, y, ax, ay, make_var(x, CHUNKS, ax, pad=fill), make_var(y, CHUNKS, ay, pad=fill)


def _sweep_cases():
    k = 0
    for (dtx, dty), (iname, index), axis, masked in itertools.product(PAIRS, INDEXES, AXES, (False, True)):
        method, ddof = METHODS[k % 3]   # every pair / index / axes / mask once; the three results rotate
        k += 1
        yield pytest.param(dtx, dty, iname, index, axis, masked, method, ddof,
                           id=f"{dtx[1:]}{dty[0].replace('|', '=')}{dty[1:]}-{iname}-"
                              f"{'all' if axis is None else ''.join(map(str, axis))}-"
                              f"{'masked' if masked else 'plain'}-{method}{ddof}")


@pytest.mark.parametrize("dtx,dty,iname,index,axis,masked,method,ddof", list(_sweep_cases()))
def test_sweep(gpu, dtx, dty, iname, index, axis, masked, method, ddof):
    x, y, ax, ay, vx, vy = sweep_vars(dtx, dty, masked)
    got = query(vx, vy, method, axis, ddof, index)
    check(got, oracle(x, y, ax, ay, NUMPY_INDEX.get(iname, index), axis), method, ddof)


# -- 2. vector-load edges and layouts --------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_vars(which, dt="<f4"):
    rng = np.random.default_rng(7)
    shape = (33, 65, 31) if which == "one" else (64, 64, 16)
    x = rng.normal(288.0, 10.0, shape)
    y = (0.3 * x + rng.normal(0.0, 5.2, shape)).astype(dt)
    x = x.astype(dt)
    if which == "one":      # a single chunk: unroll step, 16-byte head and tail, tile merge
        return x, y, make_var(x, shape), make_var(y, shape)
    sx, sy = {"xshuf": (True, False), "yshuf": (False, True), "both": (True, True)}[which]
    return x, y, make_var(x, (32, 64, 16), shuffle=sx), make_var(y, (32, 64, 16), shuffle=sy)


@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None), slice(None), slice(None))], ids=["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
@pytest.mark.parametrize("which,dt", [("one", "<f4"), ("xshuf", "<f4"), ("yshuf", "<f4"), ("both", "<f8"),
                                      ("xshuf", "<i2")])
def test_vector_edges_and_layouts(gpu, which, dt, axis, index):
    x, y, vx, vy = edge_vars(which, dt)
    o = oracle(x, y, None, None, index, axis)
    check(query(vx, vy, "cov", axis, 1, index), o, "cov", 1)
    check(query(vx, vy, "corr", axis, 0, index), o, "corr")


def _full_records(gpu, x, y, off_x, off_y, index=None):
    """pyas_comoments_axes over every dim of one chunk per side, each side's
    chunk ``off`` bytes into its own buffer."""
    from pyactivestorage_amd import selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    st = gpu.thread_stream()
    bufs, plans = [], []
    for data, off in ((x, off_x), (y, off_y)):
        buf = DeviceBuffer(gpu, data.nbytes + 64)
        host = np.zeros(data.nbytes + 64, np.uint8)
        host[off:off + data.nbytes] = np.frombuffer(data.tobytes(), np.uint8)
        gpu.h2d(buf.ptr, host, st)
        sels = None if index is None else [selection.normalize(index, data.shape)]
        plans.append(ReductionPlan(gpu, data.dtype, data.shape, buf.ptr, np.array([off], np.int64), selections=sels,
                                   missing=(None,) * 4, stream=st))
        bufs.append(buf)
    out = np.zeros(1, engine.comoments_dtype)
    obuf = DeviceBuffer(gpu, out.nbytes)
    engine.comoments_axes(gpu, plans[0].batch, plans[0].mask_up.struct, plans[1].batch, plans[1].mask_up.struct,
                          (1 << x.ndim) - 1, None, obuf.ptr, st)
    gpu.d2h(out, obuf.ptr, st)
    gpu.synchronize(st)
    return out


@pytest.mark.parametrize("off_x,off_y", [(0, 4), (4, 0), (4, 4), (8, 12)], ids=["y4", "x4", "both4", "x8y12"])
def test_bases_misaligned(gpu, off_x, off_y):
    """The two chunk bases misaligned differently: the full kernel's
    per-element fallback; alike: its vector path with a head and a tail.  All
    give the record of the aligned run within tolerance.  (Through the entry
    point itself: ``attach_resident`` takes 256-byte aligned slots only.)"""
    x, y, _, _ = edge_vars("one")
    for index in (None, (slice(1, None), slice(None), slice(0, 31))):
        got = _full_records(gpu, x, y, off_x, off_y, index)
        o = oracle(x, y, None, None, Ellipsis if index is None else index, None)
        assert int(got["count"][0]) == int(o["n"].reshape(-1)[0])
        check(comoments.finalize_cov(got.reshape(1, 1, 1), 0), o, "cov", 0, f"offsets {off_x} {off_y}")
        check(comoments.finalize_corr(got.reshape(1, 1, 1)), o, "corr", 0, f"offsets {off_x} {off_y}")


def test_small_tiles_merge_in_order(gpu):
    """More than one tile per chunk (and a tile boundary inside the run)."""
    x, y, vx, vy = edge_vars("one")
    o = oracle(x, y, None, None, (Ellipsis,), None)
    base = query(vx, vy, "cov", None, 0, (Ellipsis,))
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        got = query(vx, vy, "cov", None, 0, (Ellipsis,))
        cut = query(vx, vy, "corr", None, 0, (slice(1, None),))
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)
    check(got, o, "cov")
    check(base, o, "cov")
    check(cut, oracle(x, y, None, None, (slice(1, None),), None), "corr")


# -- 3. more than 64 chunks in a full reduction: two levels of the fold ---------------
def test_hundred_chunks(gpu):
    rng = np.random.default_rng(13)
    x = rng.normal(288.0, 10.0, (40, 40, 5)).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 5.2, x.shape)).astype("<f4")
    vx, vy = make_var(x, (4, 4, 5)), make_var(y, (4, 4, 5))
    o = oracle(x, y, None, None, Ellipsis, None)
    check(query(vx, vy, "cov", None, 1, Ellipsis), o, "cov", 1)
    check(query(vx, vy, "corr", None, 0, Ellipsis), o, "corr")
    o = oracle(x, y, None, None, Ellipsis, (0, 1))
    check(query(vx, vy, "cov", (0, 1), 0, Ellipsis), o, "cov", 0)


# -- 4. exactness ------------------------------------------------------------------
def test_constant_side_is_exactly_zero(gpu):
    rng = np.random.default_rng(17)
    x = np.full((20, 30, 17), 287.65, "<f4")
    y = rng.normal(10.0, 3.0, x.shape).astype("<f4")
    vx, vy = make_var(x, (8, 12, 20), pad=1.0), make_var(y, (8, 12, 20))
    for axis in (None, (0,), (2,), (0, 2)):
        for a, b in ((vx, vy), (vy, vx)):
            got = query(a, b, "cov", axis, 0, Ellipsis)
            assert not np.ma.getmaskarray(got).any()
            assert (got.data == 0.0).all(), (axis, got)
            r = query(a, b, "corr", axis, 0, Ellipsis)
            assert not np.ma.getmaskarray(r).any() and np.isnan(r.data).all(), (axis, r)


@pytest.mark.parametrize("axis", [None, (0,), (2,), (0, 2)], ids=["all", "0", "2", "02"])
def test_self_and_linear(gpu, axis):
    x, _, ax, _, vx, _ = sweep_vars("<f4", "<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))
    twin = make_var(x, CHUNKS, ax, pad=-999.0)             # a second Active over the same data
    var = Active(vx).var(axis=axis, ddof=1)[index]
    for same, vy in ((True, vx), (False, twin)):
        r = query(vx, vy, "corr", axis, 0, index, same=same)
        assert not np.ma.getmaskarray(r).any()
        assert np.abs(r.data - 1.0).max() <= TOL
        c = query(vx, vy, "cov", axis, 1, index, same=same)
        assert np.array_equal(np.ma.getmaskarray(c), np.ma.getmaskarray(var))
        np.testing.assert_allclose(c.data, var.data, rtol=1e-9, atol=0)
    y = (-2.0 * x).astype("<f4")                             # exact in f32
    ay = {"_FillValue": np.array([1998.0], "<f4")}           # -2 x (-999): x's fill positions
    r = query(vx, make_var(y, CHUNKS, ay, pad=1998.0), "corr", axis, 0, index)
    assert not np.ma.getmaskarray(r).any()
    assert np.abs(r.data + 1.0).max() <= TOL


# -- 5. conditioning -----------------------------------------------------------------
def test_conditioning(gpu):
    """f4 1e6 + U(0, 1) against an independent draw of the same:
    ``sum x y - sum x sum y / n`` loses every digit here."""
    rng = np.random.default_rng(21)
    x = (1e6 + rng.uniform(0, 1, (32, 32, 32))).astype("<f4")
    y = (1e6 + rng.uniform(0, 1, (32, 32, 32))).astype("<f4")
    vx, vy = make_var(x, (16, 32, 32)), make_var(y, (16, 32, 32))
    for axis in (None, (0,), (2,)):
        o = oracle(x, y, None, None, Ellipsis, axis)
        check(query(vx, vy, "cov", axis, 1, Ellipsis), o, "cov", 1, f"offset {axis}")
        check(query(vx, vy, "corr", axis, 0, Ellipsis), o, "corr", 0, f"offset {axis}")


# -- 6. masked edge cases ----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked_vars():
    rng = np.random.default_rng(31)
    x = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 1.5, x.shape)).astype("<f4")
    x[0:4, 0:6, 0:5] = -999.0             # one chunk entirely fill values, in x only
    x[:, 7, 3] = -999.0                   # an axis-0 output masked in x only
    y[:, 7, 4] = -777.0                   # and one masked in y only
    x[:, 8, 2] = -999.0                   # an output with exactly one pair:
    x[5, 8, 2] = 12.5                     #   x leaves one element,
    y[:4, 9, 2] = -777.0                  #   and x, y leave different ones but one in common
    x[4:, 9, 2] = -999.0
    x[4, 9, 2] = 11.0
    ax = {"_FillValue": np.array([-999.0], "<f4")}
    ay = {"_FillValue": np.array([-777.0], "<f4")}
    return x, y, ax, ay, make_var(x, (4, 6, 5), ax), make_var(y, (4, 6, 5), ay)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("axis", [None, (0,), (1,), (2,), (0, 2)], ids=["all", "0", "1", "2", "02"])
def test_masked_edges(gpu, axis, ddof):
    x, y, ax, ay, vx, vy = masked_vars()
    o = oracle(x, y, ax, ay, Ellipsis, axis)
    cov = query(vx, vy, "cov", axis, ddof, Ellipsis)
    corr = query(vx, vy, "corr", axis, 0, Ellipsis)
    check(cov, o, "cov", ddof)
    check(corr, o, "corr")
    if axis == (0,):
        m = np.ma.getmaskarray(cov)
        assert m[0, 7, 3] and m[0, 7, 4] and not m[0, 7, 2] and not m[0, 6, 3]
        assert np.ma.getmaskarray(corr)[0, 7, 3] and np.ma.getmaskarray(corr)[0, 7, 4]
        assert o["n"][0, 8, 2] == 1 and o["n"][0, 9, 2] == 1
        for j in (8, 9):
            if ddof == 0:
                assert not m[0, j, 2] and cov.data[0, j, 2] == 0.0
            else:
                assert m[0, j, 2]
            assert not np.ma.getmaskarray(corr)[0, j, 2] and np.isnan(corr.data[0, j, 2])


def test_all_masked_selection(gpu):
    x, y, ax, ay, vx, vy = masked_vars()
    index = (slice(0, 4), slice(0, 6), slice(0, 5))
    for axis in (None, (1,)):
        for method in ("cov", "corr"):
            got = query(vx, vy, method, axis, 0, index)
            assert np.ma.getmaskarray(got).all() and got.dtype == np.float64
            assert got.shape == ((1, 1, 1) if axis is None else (4, 1, 5))


@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_vector_missing_value(gpu, axis, side):
    """A vector ``missing_value`` on one side (broadcast over the last dim of
    each chunk's selection), a scalar ``_FillValue`` on the other: per-chunk
    selections and host-built segments, each side's table walked by the same
    selection position."""
    rng = np.random.default_rng(41)
    a = rng.normal(10.0, 3.0, (8, 6, 10)).astype("<f4")
    b = (0.3 * a + rng.normal(0.0, 1.5, a.shape)).astype("<f4")
    vec = np.array([1.0, 2.0, 3.0, 4.0, 5.0], "<f4")
    hit = rng.random(a.shape) < 0.1
    a[hit] = np.broadcast_to(np.tile(vec, 2), a.shape)[hit]
    b[rng.random(b.shape) < 0.05] = -777.0
    attrs_a, attrs_b = {"missing_value": vec}, {"_FillValue": np.array([-777.0], "<f4")}
    miss_a, miss_b = (None, np.tile(vec, 2), None, None), None   # the same rule over the whole selection
    va, vb = make_var(a, (4, 3, 5), attrs_a), make_var(b, (4, 3, 5), attrs_b)
    if side == "x":
        o = oracle(a, b, None, attrs_b, Ellipsis, axis, missing_x=miss_a)
        args = (va, vb)
    else:
        o = oracle(b, a, attrs_b, None, Ellipsis, axis, missing_y=miss_a)
        args = (vb, va)
    check(query(*args, "cov", axis, 1, Ellipsis), o, "cov", 1)
    check(query(*args, "corr", axis, 0, Ellipsis), o, "corr")


# -- 7. non-finite ------------------------------------------------------------------------
def test_non_finite(gpu):
    """An unmasked NaN, +inf and -inf (in different chunks, each in one side
    only) give NaN where the oracle has NaN; every other output is unaffected."""
    rng = np.random.default_rng(51)
    x = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 1.5, x.shape)).astype("<f4")
    x[1, 2, 3] = np.nan
    y[6, 9, 7] = np.inf
    x[2, 8, 1] = -np.inf
    vx, vy = make_var(x, (4, 6, 5)), make_var(y, (4, 6, 5))
    for axis in (None, (0,), (2,), (0, 2)):
        o = oracle(x, y, None, None, Ellipsis, axis)
        assert np.isnan(_plain(o["cxy"])).sum() == (1 if axis is None else 3)
        check(query(vx, vy, "cov", axis, 0, Ellipsis), o, "cov", 0, f"{axis}")
        check(query(vx, vy, "corr", axis, 0, Ellipsis), o, "corr", 0, f"{axis}")


# -- 8. components ---------------------------------------------------------------------------
def test_components_merge(gpu):
    x, y, ax, ay, vx, vy = sweep_vars("<f4", "<f4", True)

    def comps(index, axis=(0,)):
        a = Active(vx, axis=axis)
        a.components = True
        return a.cov(Active(vy))[index]

    whole, lo, hi = comps(Ellipsis), comps(slice(0, 8)), comps(slice(8, None))
    names = ["cxy", "m2_x", "m2_y", "mean_x", "mean_y", "n"]
    assert sorted(whole) == names
    assert whole["n"].dtype == np.int64 and not np.ma.getmaskarray(whole["n"]).any()
    for k in names[:-1]:
        assert whole[k].dtype == np.float64 and whole[k].shape == (1, 22, 37)
        assert np.array_equal(np.ma.getmaskarray(whole[k]), np.ma.getdata(whole["n"]) == 0)
    o = oracle(x, y, ax, ay, Ellipsis, (0,))
    np.testing.assert_array_equal(np.ma.getdata(whole["n"]), o["n"])
    np.testing.assert_allclose(_plain(whole["mean_x"]), _plain(o["mean_x"]), rtol=1e-12)
    np.testing.assert_allclose(_plain(whole["m2_y"]), _plain(o["m2_y"]), rtol=TOL)
    rec = lambda c: comoments.records(np.ma.getdata(c["n"]), *(np.ma.getdata(c[k]) for k in
                                                                ("mean_x", "mean_y", "m2_x", "m2_y", "cxy")))
    merged = comoments.merge(rec(lo), rec(hi))
    np.testing.assert_array_equal(merged["count"], np.ma.getdata(whole["n"]))
    check(comoments.finalize_cov(merged, 1), o, "cov", 1, "merged halves")
    check(comoments.finalize_corr(merged), o, "corr", 0, "merged halves")
    check(comoments.finalize_cov(rec(whole), 1), o, "cov", 1, "whole")
    # the regression slope of y on x named in the docstring
    with np.errstate(all="ignore"):
        slope = np.ma.getdata(whole["cxy"]) / np.ma.getdata(whole["m2_x"])
    assert abs(np.nanmedian(slope) - 0.3) < 0.1


# -- 9. determinism and residency ------------------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_deterministic_and_resident(gpu, axis):
    x, y, ax, ay, vx, vy = sweep_vars("<f4", "<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))

    def run(res_x, res_y, method="cov"):
        a, b = Active(vx, axis=axis, resident=res_x), Active(vy, resident=res_y)
        return getattr(a, method)(b)[index]

    first = run(False, False)
    assert _bytes(run(False, False)) == _bytes(first)
    corr = run(False, False, "corr")
    try:
        for res_x, res_y in ((True, False), (False, True), (True, True), (True, True)):
            assert _bytes(run(res_x, res_y)) == _bytes(first), (res_x, res_y)
        assert _bytes(run(True, True, "corr")) == _bytes(corr)
        # the resident stores serve the single-variable queries as before
        assert _bytes(Active(vx, axis=axis, resident=True).var()[index]) == _bytes(Active(vx, axis=axis).var()[index])
    finally:
        release_resident(vx)
        release_resident(vy)
    assert vx._pyas_resident is None and vy._pyas_resident is None


# -- 10. the C entry point's argument checks ----------------------------------------------------
def test_entry_point_errors(gpu):
    def batch(dtype=_lib.F32, shape=(4, 4), n=1):
        b = _lib.Batch()
        b.dtype, b.ndim, b.n_chunks = dtype, len(shape), n
        for d, s in enumerate(shape):
            b.chunk_shape[d] = s
        b.data, b.offsets = 256, 256      # never dereferenced: every call below fails its checks
        return b

    def call(bx, by, axes=3, out=8):
        m = _lib.Mask()
        return gpu.lib.pyas_comoments_axes(gpu.handle, None if bx is None else ctypes.byref(bx), ctypes.byref(m),
                                           None if by is None else ctypes.byref(by), ctypes.byref(m), axes, None,
                                           out, None)

    assert call(None, batch()) == _lib.EINVAL
    assert call(batch(), None) == _lib.EINVAL
    assert call(batch(), batch(shape=(4, 5))) == _lib.EINVAL
    assert call(batch(), batch(shape=(4, 4, 1))) == _lib.EINVAL
    assert call(batch(), batch(n=2)) == _lib.EINVAL
    assert call(batch(), batch(dtype=_lib.F64)) == _lib.ENOTSUP
    assert call(batch(), batch(dtype=_lib.I32)) == _lib.ENOTSUP
    assert call(batch(), batch(), axes=4) == _lib.EINVAL           # axes beyond the rank
    assert call(batch(), batch(), out=None) == _lib.EINVAL
    assert call(batch(), batch(), axes=1) == _lib.EINVAL           # partial axes need out_offsets
    nine = batch()
    nine.ndim = 9
    assert call(nine, nine) == _lib.ENOTSUP
    g = _lib.Grid()
    g.ndim = 0
    assert gpu.lib.pyas_comoments_combine_grid(gpu.handle, 8, ctypes.byref(g), 8, None) == _lib.ENOTSUP
    assert gpu.lib.pyas_comoments_combine_segments(gpu.handle, None, None, None, 1, None, None) == _lib.EINVAL


# -- 11. branches the shapes above do not reach (the cases of tests/_stats_gaps.py) -----------
from tests import _stats_gaps as G   # noqa: E402

MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
LAYOUTS = {"xshuf": (True, False), "yshuf": (False, True), "both": (True, True), "plain": (False, False)}


@functools.lru_cache(maxsize=None)
def gap_vars(group, name, dt="<f4", masked=False, layout=None):
    """The case's pair; masked: the two sides have their fill values at different positions."""
    x, y, ax, ay = G.pair(group, name, dt, masked)
    _, chunks, _, _, shuffled = G.case(group, name)
    sx, sy = LAYOUTS[layout or ("both" if shuffled else "plain")]
    return (x, y, ax, ay, make_var(x, chunks, ax, shuffle=sx, pad=G.fill_of(ax, dt)),
            make_var(y, chunks, ay, shuffle=sy, pad=G.fill_of(ay, dt)))


def gap_check(group, name, dt, masked, iname, axis, layout=None):
    x, y, ax, ay, vx, vy = gap_vars(group, name, dt, masked, layout)
    index = G.index_of(group, name, iname)
    o = oracle(x, y, ax, ay, index, axis)
    what = f"{group} {name} {dt} {layout or ''} {iname} {G.axis_id(axis)}"
    check(query(vx, vy, "cov", axis, 1, index), o, "cov", 1, what)
    check(query(vx, vy, "corr", axis, 0, index), o, "corr", 0, what)


@MASKED
@pytest.mark.parametrize("name,iname", [(n, i) for n in G.G1 for i in G.case("G1", n)[3]])
def test_g1_reduced_positions_beyond_the_offset_map(gpu, name, iname, masked):
    """More than kComRoff reduced positions in a chunk: the radix-counter walk
    of k_comoments_axes, a wave ("row") and a lane ("lane") per output."""
    gap_check("G1", name, "<f4", masked, iname, G.case("G1", name)[2][0])


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(gpu, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in its launch."""
    x, y, ax, ay, vx, vy = gap_vars("G2", name, "<f4", masked)
    k = G.G2_SECOND_TRIP
    o = oracle(x, y, ax, ay, Ellipsis, (0,))
    tail = {key: v.reshape(-1)[k:] for key, v in o.items()}
    for method, ddof in (("cov", 1), ("corr", 0)):
        got = query(vx, vy, method, (0,), ddof, Ellipsis)
        assert got.shape == (1, 130, 130)
        check(got.reshape(-1)[k:], tail, method, ddof, f"G2 {name}: the second trip, outputs {k}..16899")
        check(got, o, method, ddof, f"G2 {name}: every output")


@MASKED
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=G.axis_id)
@pytest.mark.parametrize("layout", ["xshuf", "yshuf", "both"])
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_shuffled_chunks_of_odd_size(gpu, dt, layout, axis, masked):
    """Shuffled chunks of 105 elements on either side or both: the
    per-element fallback of the shuffled co-moment runs."""
    for iname in ("whole", "from1"):
        gap_check("G3", "odd", dt, masked, iname, axis, layout)


@pytest.mark.parametrize("iname", list(G.G3_RUNS))
@pytest.mark.parametrize("layout", ["xshuf", "yshuf", "both"])
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_runs_inside_a_shuffled_chunk(gpu, dt, layout, iname):
    gap_check("G3", "runs", dt, False, iname, None, layout)


@MASKED
@pytest.mark.parametrize("name", list(G.G4))
def test_g4_ranks(gpu, name, masked):
    for iname, _, axis, _ in G.combos("G4", name):
        gap_check("G4", name, "<f4", masked, iname, axis)


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    for axis in (None, (1,)):
        gap_check("G5", "dtypes", dt, masked, "whole", axis, "both" if shuffle else "plain")
