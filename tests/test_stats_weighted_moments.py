"""``Active.var`` / ``std`` / ``cov`` / ``corr`` with ``weights=`` on the
device against NumPy.

Oracle (two passes, independent of the device's walk): ``x[index]`` (and
``y[index]``) taken with NumPy, each masked with
``oracle.storage_ref.mask_missing`` under its own attributes, the common mask
their OR, values converted with ``astype(float64)``; ``W`` the outer product of
the weight vectors taken at the selected global indices in ascending dim
order, 0 where masked (as ``test_gpu_weighted.oracle`` builds it).  Per output,
about the smallest counted value of positive weight (the moments do not depend
on the origin; with it, equal values and an output of one positive weight have
deviations of exactly 0, as in exact arithmetic): ``sw``, ``sw2``, the
weighted means, ``m2_x = sum W (x - mean_x)^2``, ``m2_y`` and ``cxy``.  For
``axis=None`` the oracle itself is checked against ``np.cov(aweights=)`` at
1e-12.

Bounds (the argument of 6.7 with non-negative terms
``w (x - K)^2`` and K a counted value of positive weight):

    var, std      1e-9 relative
    cov           1e-9 sqrt(m2_x m2_y) / fact,  fact = (sw sw - ddof sw2) / sw
    corr          1e-9 absolute
    sw, sw2       4 (n_sel + 8) 2^-53 relative (non-negative terms)

Mask, ``n`` and NaN positions are exact; the dtype is float64.  The oracle
asserts on the CPU that the data lie within 6 sigma of their mean and that
every output not meant to be masked has ``(sw^2 - ddof sw2) / sw^2 >= 1e-6``,
so a mask never hangs on a rounding.  Each check prints its largest error over
its bound.
"""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import _lib, engine, wmoments
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import get_missing_attributes
from tests import _stats_gaps as G
from tests import test_gpu_comoments as C
from tests import test_gpu_weighted as WT
from tests.test_gpu_comoments import make_var

pytestmark = pytest.mark.gpu

TOL = 1e-9
U = 2.0 ** -53
WORST = {"var": 0.0, "std": 0.0, "cov": 0.0, "corr": 0.0}    # the largest errors seen, in units of the bounds


# -- the oracle ---------------------------------------------------------------------------------
def _per_dim(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    if Ellipsis in index:
        k = index.index(Ellipsis)
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def oracle(x, y, attrs_x, attrs_y, index, axis, weights, missing_x=None, sigma=True):
    """n, sw, sw2, the weighted means, m2_x, m2_y and cxy (``keepdims``
    shapes) of the elements of ``x`` (pairs with ``y``, unless it is None)
    unmasked on both sides, and ``n_sel``, the selected elements per output."""
    nd = x.ndim
    xs = ref.mask_missing(x[index], missing_x or get_missing_attributes(attrs_x or {}))
    m = np.ma.getmaskarray(xs)
    sides = {"x": np.ma.getdata(xs)}
    if y is not None:
        ys = ref.mask_missing(y[index], get_missing_attributes(attrs_y or {}))
        m = m | np.ma.getmaskarray(ys)
        sides["y"] = np.ma.getdata(ys)
    ok = ~m
    W = np.ones(m.shape)
    for d, ix in enumerate(_per_dim(index, nd)):          # ascending dimension order
        if d in weights:
            w = np.asarray(weights[d], np.float64)[np.arange(x.shape[d])[ix]]
            W = W * w.reshape([-1 if k == d else 1 for k in range(nd)])
    W = np.where(ok, W, 0.0)
    axis = tuple(range(nd)) if axis is None else axis
    kw = dict(axis=axis, keepdims=True)
    o = {"n": ok.sum(**kw), "n_sel": int(np.prod([m.shape[a] for a in axis]))}
    with np.errstate(all="ignore"):
        o["sw"], o["sw2"] = W.sum(**kw), (W * W).sum(**kw)
        sw = np.where(o["sw"] == 0, 1.0, o["sw"])
        dev = {}
        for s, v in sides.items():
            v = np.where(ok, v.astype(np.float64), 0.0)
            pos = ok & (W > 0) & np.isfinite(v)
            origin = np.where(pos, v, np.inf).min(**kw)
            origin = np.where(np.isfinite(origin), origin, 0.0)
            d = np.where(ok, v - origin, 0.0)
            mean = (W * d).sum(**kw) / sw
            dev[s] = np.where(ok, d - mean, 0.0)
            o["mean_" + s] = origin + mean
            o["m2_" + s] = (W * dev[s] * dev[s]).sum(**kw)
            if sigma and pos.any():   # the selection's data lie within 6 sigma of their weighted mean
                mu = (W * v)[pos].sum() / W[pos].sum()
                sd = np.sqrt((W * (v - mu) ** 2)[pos].sum() / W[pos].sum())
                assert np.abs(v[pos] - mu).max() <= 6.0 * sd, (s, float(np.abs(v[pos] - mu).max() / sd))
        if y is not None:
            o["cxy"] = (W * dev["x"] * dev["y"]).sum(**kw)
    # no mask hangs on a rounding
    for ddof in (0, 1):
        num = o["sw"] * o["sw"] - ddof * o["sw2"]
        live = (o["sw"] > 0) & (num != 0)
        assert (num[live] / (o["sw"][live] ** 2) >= 1e-6).all()
    if len(axis) == nd and int(o["n"].reshape(-1)[0]) >= 2:   # the oracle itself against np.cov(aweights=)
        sel = ok & (W > 0)
        cols = [np.where(ok, v.astype(np.float64), 0.0)[sel] for v in sides.values()]
        if all(np.isfinite(c).all() and c.std() > 0 for c in cols) and sel.sum() >= 2 \
                and all(np.isfinite(o[k]).all() for k in o if k.startswith("m2_")):
            for ddof in (0, 1):
                c = np.atleast_2d(np.cov(*cols, aweights=W[sel], ddof=ddof))
                fact = float(((o["sw"] ** 2 - ddof * o["sw2"]) / o["sw"]).reshape(-1)[0])
                m2x = float(o["m2_x"].reshape(-1)[0])
                assert abs(m2x / fact - c[0, 0]) <= 1e-12 * c[0, 0]
                if y is not None:
                    m2y, cxy = float(o["m2_y"].reshape(-1)[0]), float(o["cxy"].reshape(-1)[0])
                    assert abs(cxy / fact - c[0, 1]) <= 1e-12 * np.sqrt(m2x * m2y) / fact
    return o


def check(got, o, method, ddof=0, what=""):
    """``got`` (a var, std, cov or corr result) against the oracle's components."""
    assert isinstance(got, np.ma.MaskedArray), what
    n, sw, sw2 = o["n"], o["sw"], o["sw2"]
    assert got.dtype == np.float64 and got.shape == n.shape, (what, got.shape, n.shape)
    with np.errstate(all="ignore"):
        num = sw * sw - ddof * sw2
        wm = (sw == 0) if method == "corr" else (sw == 0) | ~(num > 0)
        fact = np.where(wm, 1.0, num / np.where(sw == 0, 1.0, sw))
        if method in ("var", "std"):
            want = o["m2_x"] / fact
            want = np.sqrt(want) if method == "std" else want
            bound = TOL * np.abs(want)
        elif method == "cov":
            want, bound = o["cxy"] / fact, TOL * np.sqrt(o["m2_x"] * o["m2_y"]) / fact
        else:
            want = np.clip(o["cxy"] / np.sqrt(o["m2_x"]) / np.sqrt(o["m2_y"]), -1.0, 1.0)
            bound = np.full(n.shape, TOL)
    assert np.array_equal(np.ma.getmaskarray(got), wm), (what, np.ma.getmaskarray(got).sum(), wm.sum())
    g, w, b = got.data[~wm], want[~wm], bound[~wm]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), (what, np.isnan(g).sum(), nan.sum())
    err = np.abs(g[~nan] - w[~nan])
    okk = err <= b[~nan]
    rel = float((err / np.where(b[~nan] > 0, b[~nan], 1.0))[b[~nan] > 0].max(initial=0.0))
    WORST[method] = max(WORST[method], rel)
    print(what, method, ddof, "largest error over its bound", rel, "(largest so far", WORST[method], ")")
    assert okk.all(), (what, method, float(err.max()), float(b[~nan][~okk].min()))


def check_sums(comp, o, what=""):
    """``sum_of_weights`` / ``sum_of_weights2`` / ``n`` of a components result."""
    np.testing.assert_array_equal(np.ma.getdata(comp["n"]), o["n"])
    for key, name in (("sum_of_weights", "sw"), ("sum_of_weights2", "sw2")):
        err = np.abs(np.ma.getdata(comp[key]) - o[name])
        bound = 4 * (o["n_sel"] + 8) * U * o[name]
        print(what, key, "largest error over its bound", float((err / np.where(bound > 0, bound, 1.0)).max()))
        assert (err <= bound).all(), (what, key)


def query(vx, vy, method, axis, ddof, weights, index, same=False, **kw):
    a = Active(vx, **kw)
    if method in ("var", "std"):
        getattr(a, method)(axis=axis, ddof=ddof, weights=weights)
    elif method == "cov":
        a.cov(a if same else Active(vy, **kw), axis=axis, ddof=ddof, weights=weights)
    else:
        a.corr(a if same else Active(vy, **kw), axis=axis, weights=weights)
    return a[index]


def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


def both(vx, vy, x, y, ax, ay, index, axis, w, what="", nindex=None, **okw):
    """A var and a std query of x against its oracle, a cov (ddof 1) and a
    corr query of the pair against theirs; both oracles."""
    nindex = index if nindex is None else nindex
    o1, o2 = oracle(x, None, ax, None, nindex, axis, w, **okw), oracle(x, y, ax, ay, nindex, axis, w, **okw)
    check(query(vx, None, "var", axis, 0, w, index), o1, "var", 0, what)
    check(query(vx, None, "std", axis, 1, w, index), o1, "std", 1, what)
    check(query(vx, vy, "cov", axis, 1, w, index), o2, "cov", 1, what)
    check(query(vx, vy, "corr", axis, 0, w, index), o2, "corr", 0, what)
    return o1, o2


# -- 1. sweep ---------------------------------------------------------------------------------------
SHAPE, CHUNKS = C.SHAPE, C.CHUNKS                     # (15, 22, 37) in chunks (8, 12, 20)
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8"]
INDEXES = C.INDEXES                                   # all / inner / stride / list / neg
AXES = [None, (0,), (2,), (0, 2), (1, 2)]
WSETS = [(2,), (1, 2), (0,)]
METHODS = [("var", 0), ("std", 1), ("cov", 1), ("corr", 0), ("var", 1), ("cov", 0), ("std", 0)]


def sweep_pair(dt, masked):
    """(x, y, attrs_x, attrs_y, var_x, var_y) with x of dtype ``dt``: the pairs
    of the co-moment sweep (``>f4``: its big-endian side is x here)."""
    if dt == ">f4":
        x, y, ax, ay, vx, vy = C.sweep_vars("<f4", ">f4", masked)
        return y, x, ay, ax, vy, vx
    return C.sweep_vars(dt, dt, masked)


def wset(dims):
    """The weights of the weighted-mean sweep: dim 1's are exactly 0 at its
    first and last index."""
    return WT.wset(dims)


def _sweep_cases():
    k = 0
    for dt, (iname, index), axis, masked in itertools.product(DTYPES, INDEXES, AXES, (False, True)):
        dims, (method, ddof) = WSETS[k % 3], METHODS[k % 7]   # weight sets and the seven results rotate
        k += 1
        yield pytest.param(dt, iname, index, axis, masked, dims, method, ddof,
                           id=f"{dt[0].replace('|', '=')}{dt[1:]}-{iname}-{G.axis_id(axis)}-"
                              f"{'masked' if masked else 'plain'}-w{''.join(map(str, dims))}-{method}{ddof}")


@pytest.mark.parametrize("dt,iname,index,axis,masked,dims,method,ddof", list(_sweep_cases()))
def test_sweep(gpu, dt, iname, index, axis, masked, dims, method, ddof):
    x, y, ax, ay, vx, vy = sweep_pair(dt, masked)
    w = wset(dims)
    two = method in ("cov", "corr")
    o = oracle(x, y if two else None, ax, ay, C.NUMPY_INDEX.get(iname, index), axis, w)
    check(query(vx, vy, method, axis, ddof, w, index), o, method, ddof)


# -- 2. vector paths -----------------------------------------------------------------------------------
def edge_weights(shape):
    return WT.edge_weights(shape)


@functools.lru_cache(maxsize=None)
def edge_pair(which, dt="<f4"):
    """"one": a single (33, 65, 31) chunk (16-byte vectors straddle its rows of
    31, a run from element 1 has a head and a tail); "both" / "xshuf" /
    "yshuf": (64, 64, 16) in shuffled chunks of (32, 64, 16); "rows37": rows
    of 37 in one chunk; "short": an innermost extent of 3."""
    if which in ("one", "both", "xshuf", "yshuf"):
        return C.edge_vars(which, dt)
    rng = np.random.default_rng(71)
    shape = {"rows37": (9, 11, 37), "short": (33, 21, 3)}[which]
    x = rng.normal(288.0, 10.0, shape)
    y = (0.3 * x + rng.normal(0.0, 5.2, shape)).astype(dt)
    x = x.astype(dt)
    return x, y, make_var(x, shape), make_var(y, shape)


@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None), slice(None), slice(None))], ids=["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
@pytest.mark.parametrize("which,dt", [("one", "<f4"), ("both", "<f4"), ("both", "<f8"), ("xshuf", "<f4"),
                                      ("yshuf", "<i2"), ("rows37", "<f4"), ("rows37", "<i2"), ("short", "<f4"),
                                      ("short", "|u1")])
def test_vector_paths(gpu, which, dt, axis, index):
    x, y, vx, vy = edge_pair(which, dt)
    both(vx, vy, x, y, None, None, index, axis, edge_weights(x.shape), f"{which} {dt}")


# -- 3. ranks and the LDS cap ---------------------------------------------------------------------------
RANK_CASES = dict(WT.RANK_CASES)                      # ranks 1, 2 and 4; factors beyond kWLds ("2d-long", "1d-long")
RANK_CASES["8d"] = (G.G4["8d"][0], G.G4["8d"][1], (0, 2, 4, 6))


@functools.lru_cache(maxsize=None)
def rank_pair(name, masked):
    shape, chunks, _ = RANK_CASES[name]
    rng = np.random.default_rng(160 + sorted(RANK_CASES).index(name))
    x = rng.normal(288.0, 10.0, shape).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 5.2, shape)).astype("<f4")
    ax = ay = {}
    if masked:
        pos = rng.permutation(x.size)
        k = max(x.size // 50, 1)
        x.reshape(-1)[pos[:k]] = -999.0
        y.reshape(-1)[pos[k:2 * k]] = -777.0
        x.reshape(-1)[pos[2 * k:2 * k + 3]] = 500.0
        ax = {"_FillValue": np.array([-999.0], "<f4"), "valid_min": np.array([200.0], "<f4"),
              "valid_max": np.array([380.0], "<f4")}
        ay = {"_FillValue": np.array([-777.0], "<f4")}
    weights = {d: rng.uniform(0.1, 3.0, n) for d, n in enumerate(shape)}
    if len(shape) == 8:
        weights = {0: weights[0], 7: weights[7]}
    return x, y, ax, ay, make_var(x, chunks, ax, pad=-999.0), make_var(y, chunks, ay, pad=-777.0), weights


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None),)], ids=["whole", "from1"])
@pytest.mark.parametrize("name", sorted(RANK_CASES))
def test_ranks_and_long_rows(gpu, name, index, masked):
    x, y, ax, ay, vx, vy, w = rank_pair(name, masked)
    for axis in (None, RANK_CASES[name][2]):
        both(vx, vy, x, y, ax, ay, index, axis, w, f"{name} {axis}")


# -- 4. tiles, many chunks -----------------------------------------------------------------------------
def test_small_tiles_merge_in_order(gpu):
    """More than one tile per chunk (and tile boundaries inside rows): within
    the bounds, and the same bytes when repeated."""
    x, y, vx, vy = edge_pair("one")
    w = edge_weights(x.shape)
    cut = (slice(1, None),)
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        got = [query(vx, None, "var", None, 1, w, (Ellipsis,)) for _ in range(2)]
        cov = [query(vx, vy, "cov", None, 0, w, cut) for _ in range(2)]
        corr = query(vx, vy, "corr", None, 0, w, (Ellipsis,))
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)
    o = oracle(x, y, None, None, (Ellipsis,), None, w)
    check(got[0], o, "var", 1)
    check(corr, o, "corr")
    check(cov[0], oracle(x, y, None, None, cut, None, w), "cov", 0)
    assert _bytes(got[0]) == _bytes(got[1]) and _bytes(cov[0]) == _bytes(cov[1])


def test_hundred_chunks(gpu):
    """(40, 40, 5) in 100 chunks: two levels of the full reduction's fold."""
    rng = np.random.default_rng(13)
    x = rng.normal(288.0, 10.0, (40, 40, 5)).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 5.2, x.shape)).astype("<f4")
    vx, vy = make_var(x, (4, 4, 5)), make_var(y, (4, 4, 5))
    w = {0: rng.uniform(0.1, 3.0, 40), 2: rng.uniform(0.1, 3.0, 5)}
    both(vx, vy, x, y, None, None, Ellipsis, None, w, "100 chunks")
    both(vx, vy, x, y, None, None, Ellipsis, (0, 1), w, "100 chunks (0, 1)")


# -- 5. two bases misaligned differently, through the C entry -----------------------------------------
def _full_records(gpu, x, y, off_x, off_y, w, index=None):
    """pyas_wcomoments_axes over every dim of one chunk per side, each side's
    chunk ``off`` bytes into its own buffer; ``y`` None: one variable."""
    from pyactivestorage_amd import selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    st = gpu.thread_stream()
    bufs, plans = [], []
    for data, off in ((x, off_x), (y, off_y)):
        if data is None:
            continue
        buf = DeviceBuffer(gpu, data.nbytes + 64)
        host = np.zeros(data.nbytes + 64, np.uint8)
        host[off:off + data.nbytes] = np.frombuffer(data.tobytes(), np.uint8)
        gpu.h2d(buf.ptr, host, st)
        sels = None if index is None else [selection.normalize(index, data.shape)]
        plans.append(ReductionPlan(gpu, data.dtype, data.shape, buf.ptr, np.array([off], np.int64), selections=sels,
                                   missing=(None,) * 4, stream=st))
        bufs.append(buf)
    pool = np.concatenate([np.asarray(w[d], np.float64) for d in range(x.ndim)])
    origin = np.zeros((1, _lib.MAX_DIMS), np.int32)
    origin[0, :x.ndim] = np.concatenate([[0], np.cumsum(x.shape)[:-1]])
    wbuf, gbuf = DeviceBuffer(gpu, pool.nbytes), DeviceBuffer(gpu, origin.nbytes)
    gpu.h2d(wbuf.ptr, pool, st)
    gpu.h2d(gbuf.ptr, origin, st)
    out = np.zeros(1, engine.wcomoments_dtype)
    obuf = DeviceBuffer(gpu, out.nbytes)
    by, my = (plans[1].batch, plans[1].mask_up.struct) if y is not None else (None, None)
    engine.wcomoments_axes(gpu, plans[0].batch, plans[0].mask_up.struct, by, my, wbuf.ptr, gbuf.ptr,
                           (1 << x.ndim) - 1, None, obuf.ptr, st)
    gpu.d2h(out, obuf.ptr, st)
    gpu.synchronize(st)
    return out


@pytest.mark.parametrize("off_x,off_y", [(0, 4), (4, 0), (4, 4), (8, 12)], ids=["y4", "x4", "both4", "x8y12"])
def test_bases_misaligned(gpu, off_x, off_y):
    """The two chunk bases misaligned differently: the per-element fallback of
    the full kernel's run; alike: its vector path with a head and a tail, and
    the position its vectors' weights start from."""
    x, y, _, _ = edge_pair("one")
    w = edge_weights(x.shape)
    for index in (None, (slice(1, None), slice(None), slice(0, 31))):
        o = oracle(x, y, None, None, Ellipsis if index is None else index, None, w)
        got = _full_records(gpu, x, y, off_x, off_y, w, index).reshape(1, 1, 1)
        assert int(got["count"][0, 0, 0]) == int(o["n"].reshape(-1)[0])
        check(wmoments.finalize_cov(got, 1), o, "cov", 1, f"offsets {off_x} {off_y}")
        check(wmoments.finalize_corr(got), o, "corr", 0, f"offsets {off_x} {off_y}")
        check(wmoments.finalize_var(got, 0), o, "var", 0, f"offsets {off_x} {off_y}")
        one = _full_records(gpu, x, None, off_x, 0, w, index).reshape(1, 1, 1)
        check(wmoments.finalize_var(one, 1, std=True), o, "std", 1, f"offset {off_x}, one variable")
        assert (one["mean_y"] == 0).all() and (one["m2_y"] == 0).all() and (one["cxy"] == 0).all()


# -- 6. exactness -------------------------------------------------------------------------------------
def test_constant_data_gives_exactly_zero(gpu):
    rng = np.random.default_rng(17)
    x = np.full((20, 30, 17), 287.65, "<f4")
    y = rng.normal(10.0, 3.0, x.shape).astype("<f4")
    vx, vy = make_var(x, (8, 12, 20), pad=1.0), make_var(y, (8, 12, 20))
    for dims in ((2,), (0, 1, 2), (1,)):
        w = {d: rng.uniform(0.0, 3.0, x.shape[d]) for d in dims}
        for axis in (None, (0,), (2,), (0, 2)):
            for method, ddof in (("var", 0), ("var", 1), ("std", 1)):
                got = query(vx, None, method, axis, ddof, w, Ellipsis)
                assert not np.ma.getmaskarray(got).any() and (got.data == 0.0).all(), (dims, axis, method)
            for a, b in ((vx, vy), (vy, vx)):
                got = query(a, b, "cov", axis, 0, w, Ellipsis)
                assert not np.ma.getmaskarray(got).any() and (got.data == 0.0).all(), (dims, axis)
                r = query(a, b, "corr", axis, 0, w, Ellipsis)
                assert not np.ma.getmaskarray(r).any() and np.isnan(r.data).all(), (dims, axis)


@pytest.mark.parametrize("axis", [None, (0,), (2,), (0, 2)], ids=["all", "0", "2", "02"])
def test_self_and_linear(gpu, axis):
    x, _, ax, _, vx, _ = C.sweep_vars("<f4", "<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))
    w = wset((0, 2))
    twin = make_var(x, CHUNKS, ax, pad=-999.0)             # a second Active over the same data
    var = query(vx, None, "var", axis, 1, w, index)
    for same, vy in ((True, vx), (False, twin)):
        r = query(vx, vy, "corr", axis, 0, w, index, same=same)
        assert not np.ma.getmaskarray(r).any()
        assert np.abs(r.data - 1.0).max() <= TOL
        c = query(vx, vy, "cov", axis, 1, w, index, same=same)
        assert np.array_equal(np.ma.getmaskarray(c), np.ma.getmaskarray(var))
        np.testing.assert_allclose(c.data, var.data, rtol=TOL, atol=0)
    y = (2.0 * x).astype("<f4")                              # exact in f32
    ay = {"_FillValue": np.array([-1998.0], "<f4")}          # 2 x (-999): x's fill positions
    r = query(vx, make_var(y, CHUNKS, ay, pad=-1998.0), "corr", axis, 0, w, index)
    assert not np.ma.getmaskarray(r).any()
    assert np.abs(r.data - 1.0).max() <= TOL


def test_conditioning(gpu):
    """The data of ``test_gpu_comoments.test_conditioning`` (f4 1e6 + U(0, 1)),
    under weights: ``sum w x x - (sum w x)^2 / sum w`` loses every digit here."""
    rng = np.random.default_rng(21)
    x = (1e6 + rng.uniform(0, 1, (32, 32, 32))).astype("<f4")
    y = (1e6 + rng.uniform(0, 1, (32, 32, 32))).astype("<f4")
    vx, vy = make_var(x, (16, 32, 32)), make_var(y, (16, 32, 32))
    w = {1: rng.uniform(0.1, 3.0, 32), 2: rng.uniform(0.1, 3.0, 32)}
    for axis in (None, (0,), (2,)):
        both(vx, vy, x, y, None, None, Ellipsis, axis, w, f"offset {axis}")


# -- 7. all-ones weights ---------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (1,), (0, 2)], ids=["all", "1", "02"])
def test_all_ones_weights_equal_the_unweighted_queries(gpu, axis):
    x, y, ax, ay, vx, vy = C.sweep_vars("<f4", "<f4", True)
    ones = {d: np.ones(n) for d, n in enumerate(SHAPE)}
    index = (slice(1, -1), slice(None), slice(2, 35))
    o1, o = both(vx, vy, x, y, ax, ay, index, axis, ones, "ones")
    for method, ddof in (("var", 0), ("var", 1), ("std", 1), ("cov", 1), ("corr", 0)):
        got = query(vx, vy, method, axis, ddof, ones, index)
        check(got, o if method in ("cov", "corr") else o1, method, ddof, "ones")   # against the oracle
        plain = query(vx, vy, method, axis, ddof, None, index)
        assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(plain)), method
        keep = ~np.ma.getmaskarray(got)
        if method in ("var", "std"):
            bound = TOL * np.abs(plain.data)
        elif method == "cov":      # fact = (sw sw - ddof sw2) / sw, which is n - ddof under weights of 1
            with np.errstate(all="ignore"):
                bound = TOL * np.sqrt(o["m2_x"] * o["m2_y"]) / ((o["sw"] ** 2 - ddof * o["sw2"]) / o["sw"])
        else:
            bound = np.full(got.shape, TOL)
        err = np.abs(got.data - plain.data)[keep]
        print("ones", method, ddof, "largest difference from the unweighted query over the bound",
              float((err / np.where(bound[keep] > 0, bound[keep], 1.0)).max(initial=0.0)))
        assert (err <= bound[keep]).all(), method              # the unweighted query's values within the bound
    for method in ("var", "cov"):
        a, b = Active(vx, axis=axis), Active(vx, axis=axis)
        a.components = b.components = True
        args = (Active(vy),) if method == "cov" else ()
        n = getattr(a, method)(*args, weights=ones)[index]["n"]
        plain = getattr(b, method)(*args)[index]["n"]
        assert np.ma.getdata(n).tobytes() == np.ma.getdata(plain).astype(np.int64).tobytes()
        np.testing.assert_array_equal(np.ma.getdata(n), (o if method == "cov" else o1)["n"])


# -- 8. zero weights ------------------------------------------------------------------------------------
def test_zero_weights(gpu):
    rng = np.random.default_rng(31)
    x = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    y = (0.3 * x + rng.normal(0.0, 1.5, x.shape)).astype("<f4")
    x[1, 2, 3] = np.nan                   # a counted NaN under weight exactly 0 (w1[2] == 0)
    x[6, 9, 7] = 1e36                     # the fill value under a positive weight
    x[3, 3, 3] = 1e36
    ax = {"_FillValue": np.array([1e36], "<f4")}
    vx, vy = make_var(x, (4, 6, 5), ax), make_var(y, (4, 6, 5))
    w1 = rng.uniform(0.5, 2.0, 12)
    w1[2] = 0.0
    w0 = np.zeros(8)
    w0[5] = 0.7                           # exactly one positive weight along dim 0
    # (a) rows of weight 0 are masked; the NaN at weight 0 gives NaN where its row is reduced with others
    w = {1: w1}
    for axis in ((0, 2), (0,), (1,), None):
        o = oracle(x, y, ax, None, Ellipsis, axis, w, sigma=False)
        for method, ddof in (("var", 0), ("std", 1), ("cov", 1), ("corr", 0)):
            got = query(vx, vy, method, axis, ddof, w, Ellipsis)
            check(got, o, method, ddof, f"zero row {axis}")
            if axis in ((0, 2), (0,)):
                assert np.ma.getmaskarray(got)[0, 2].all() and not np.ma.getmaskarray(got)[0, 3].any()
            else:
                nan = np.isnan(got.data)
                assert nan.sum() == 1 and (axis is None or nan[1, 0, 3])
            assert np.isfinite(got.data[~np.ma.getmaskarray(got) & ~np.isnan(got.data)]).all()
    # (b) exactly one positive weight: masked for ddof 1 (the numerator is exactly 0), var exactly 0 for ddof 0
    w = {0: w0}
    for method in ("var", "std", "cov"):
        got1 = query(vx, vy, method, (0,), 1, w, Ellipsis)
        assert np.ma.getmaskarray(got1).all(), method
        got0 = query(vx, vy, method, (0,), 0, w, Ellipsis)
        assert not np.ma.getmaskarray(got0).any(), method
        keep = np.ones(got0.shape, bool)
        keep[0, 2, 3] = False             # the NaN of row 1 under weight 0: NaN, not 0
        assert (got0.data[keep] == 0.0).all() and np.isnan(got0.data[0, 2, 3]), method
    corr = query(vx, vy, "corr", (0,), 0, w, Ellipsis)
    assert not np.ma.getmaskarray(corr).any() and np.isnan(corr.data).all()
    # (c) every weight 0: everything is masked
    for method in ("var", "cov", "corr"):
        got = query(vx, vy, method, (0,), 0, {0: np.zeros(8)}, Ellipsis)
        assert np.ma.getmaskarray(got).all() and got.dtype == np.float64
    # (d) the masked 1e36 under a positive weight leaves finite results
    w = {0: rng.uniform(0.5, 2.0, 8), 2: rng.uniform(0.5, 2.0, 10)}
    for axis in (None, (0,), (2,)):
        o = oracle(x, y, ax, None, Ellipsis, axis, w, sigma=False)
        for method, ddof in (("var", 1), ("cov", 0)):
            got = query(vx, vy, method, axis, ddof, w, Ellipsis)
            check(got, o, method, ddof, f"fill {axis}")
            assert np.isfinite(got.data[~np.isnan(o["m2_x"])]).all()
            assert np.isnan(got.data).sum() == 1


# -- 9. components --------------------------------------------------------------------------------------
def test_components_merge(gpu):
    x, y, ax, ay, vx, vy = C.sweep_vars("<f4", "<f4", True)
    w = wset((0, 1, 2))

    def comps(index, method, axis=(0,)):
        a = Active(vx, axis=axis)
        a.components = True
        return (a.cov(Active(vy), weights=w) if method == "cov" else a.var(weights=w))[index]

    for method, names in (("var", ["m2", "mean", "n", "sum_of_weights", "sum_of_weights2"]),
                          ("cov", ["cxy", "m2_x", "m2_y", "mean_x", "mean_y", "n", "sum_of_weights",
                                   "sum_of_weights2"])):
        o = oracle(x, y if method == "cov" else None, ax, ay, Ellipsis, (0,), w)
        whole, lo, hi = comps(Ellipsis, method), comps(slice(0, 8), method), comps(slice(8, None), method)
        assert sorted(whole) == names
        assert whole["n"].dtype == np.int64 and not np.ma.getmaskarray(whole["n"]).any()
        for k in names:
            if k != "n":
                assert whole[k].dtype == np.float64 and whole[k].shape == (1, 22, 37)
                assert np.array_equal(np.ma.getmaskarray(whole[k]), np.ma.getdata(whole["n"]) == 0)
        check_sums(whole, o, f"components {method}")

        def rec(c):
            get = lambda k: np.ma.getdata(c[k]) if k in c else 0.0
            return wmoments.records(np.ma.getdata(c["n"]), get("sum_of_weights"), get("sum_of_weights2"),
                                    get("mean" if method == "var" else "mean_x"), get("mean_y"),
                                    get("m2" if method == "var" else "m2_x"), get("m2_y"), get("cxy"))
        merged = wmoments.merge(rec(lo), rec(hi))
        np.testing.assert_array_equal(merged["count"], np.ma.getdata(whole["n"]))   # n exact
        check_sums({"n": merged["count"], "sum_of_weights": merged["sw"], "sum_of_weights2": merged["sw2"]}, o,
                   "merged halves")
        live = o["sw"] > 0
        np.testing.assert_allclose(merged["mean_x"][live], o["mean_x"][live], rtol=1e-12)
        check(wmoments.finalize_var(merged, 1), o, "var", 1, "merged halves")
        check(wmoments.finalize_var(rec(whole), 1, std=True), o, "std", 1, "whole")
        if method == "cov":
            check(wmoments.finalize_cov(merged, 1), o, "cov", 1, "merged halves")
            check(wmoments.finalize_corr(merged), o, "corr", 0, "merged halves")
            check(wmoments.finalize_cov(rec(whole), 0), o, "cov", 0, "whole")


# -- 10. determinism, residency, unweighted unchanged -------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_deterministic_and_resident(gpu, axis):
    x, y, ax, ay, vx, vy = C.sweep_vars("<f4", "<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))
    w = wset((0, 1, 2))

    def run(method, res, weights=w):
        a, b = Active(vx, axis=axis, resident=res), Active(vy, resident=res)
        if method in ("var", "std"):
            return getattr(a, method)(ddof=1, weights=weights)[index]
        return getattr(a, method)(b, weights=weights)[index]

    first = {m: run(m, False) for m in ("var", "cov", "corr")}
    for m in first:
        assert _bytes(run(m, False)) == _bytes(first[m]), m
    plain = {m: run(m, False, None) for m in ("var", "cov")}
    try:
        for m in first:
            assert _bytes(run(m, True)) == _bytes(first[m]), m
            assert _bytes(run(m, True)) == _bytes(first[m]), m          # from the resident stores
        for m in plain:
            assert _bytes(run(m, True, None)) == _bytes(plain[m]), m     # the keyword is per query
    finally:
        release_resident(vx)
        release_resident(vy)
    assert vx._pyas_resident is None and vy._pyas_resident is None


def test_unweighted_queries_unchanged(gpu):
    """A query without weights returns the bytes it did before, also right
    after a weighted one on the same object."""
    x, y, ax, ay, vx, vy = C.sweep_vars("<i2", "<i2", True)
    a, b = Active(vx, axis=(1,)), Active(vy)
    want_var, want_cov, want_mean = a.var(ddof=1)[1:-1], a.cov(b)[1:-1], a.mean()[1:-1]
    a.var(weights=wset((1,)))[1:-1]
    a.cov(b, weights=wset((1, 2)))[1:-1]
    got_var, got_cov, got_mean = a.var(ddof=1)[1:-1], a.cov(b)[1:-1], a.mean()[1:-1]
    assert _bytes(got_var) == _bytes(want_var) and _bytes(got_cov) == _bytes(want_cov)
    assert got_mean.dtype == want_mean.dtype and _bytes(got_mean) == _bytes(want_mean)


# -- 11. a netCDF file -------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (1, 2)], ids=["all", "0", "12"])
def test_netcdf_file_cos_weights(gpu, axis):
    """tas of test1.nc by file path and as a ChunkedVariable, cos-shaped
    weights on dimension 1 (the case of ``test_gpu_weighted``); the data come
    from the method=None selection."""
    from tests.test_gpu_active import variable
    path, key = os.path.join(WT.NC, "test1.nc"), "test1.nc:tas"
    sel = np.ma.asarray(Active(path, "tas")[...])
    shape = sel.shape
    w = {1: np.cos(np.linspace(-np.pi / 2, np.pi / 2, shape[1] + 2))[1:-1]}
    index = tuple(slice(n // 4, n) for n in shape)
    data = np.ma.getdata(sel)
    attrs = variable(key).attrs
    o = oracle(data, data, attrs, attrs, index, axis, w, sigma=False)
    for method, ddof in (("var", 1), ("std", 0), ("cov", 1), ("corr", 0)):
        by_path = query(path, None, method, axis, ddof, w, index, same=True, ncvar="tas")
        by_var = query(variable(key), None, method, axis, ddof, w, index, same=True)
        check(by_path, o, method, ddof, "test1.nc")
        assert _bytes(by_var) == _bytes(by_path)


# -- 12. the C entry point's argument checks -----------------------------------------------------------------
def test_entry_point_errors(gpu):
    def batch(dtype=_lib.F32, shape=(4, 4), n=1):
        b = _lib.Batch()
        b.dtype, b.ndim, b.n_chunks = dtype, len(shape), n
        for d, s in enumerate(shape):
            b.chunk_shape[d] = s
        b.data, b.offsets = 256, 256      # never dereferenced: every call below fails its checks
        return b

    def call(bx, by, axes=3, out=8, weights=(256, 256)):
        m = _lib.Mask()
        wts = None if weights is None else ctypes.byref(_lib.Weights(*weights))
        return gpu.lib.pyas_wcomoments_axes(gpu.handle, None if bx is None else ctypes.byref(bx), ctypes.byref(m),
                                            None if by is None else ctypes.byref(by), ctypes.byref(m), wts, axes,
                                            None, out, None)

    assert call(None, batch()) == _lib.EINVAL
    assert call(batch(), batch(shape=(4, 5))) == _lib.EINVAL
    assert call(batch(), batch(shape=(4, 4, 1))) == _lib.EINVAL
    assert call(batch(), batch(n=2)) == _lib.EINVAL
    assert call(batch(), batch(dtype=_lib.F64)) == _lib.ENOTSUP
    assert call(batch(), batch(dtype=_lib.I32)) == _lib.ENOTSUP
    for by in (batch(), None):                                     # two variables, one variable
        assert call(batch(), by, axes=4) == _lib.EINVAL            # axes beyond the rank
        assert call(batch(), by, out=None) == _lib.EINVAL
        assert call(batch(), by, axes=1) == _lib.EINVAL            # partial axes need out_offsets
        assert call(batch(), by, weights=None) == _lib.EINVAL
        assert call(batch(), by, weights=(None, 256)) == _lib.EINVAL
        assert call(batch(), by, weights=(256, None)) == _lib.EINVAL
    nine = batch()
    nine.ndim = 9
    assert call(nine, nine) == _lib.ENOTSUP
    assert call(nine, None) == _lib.ENOTSUP
    g = _lib.Grid()
    g.ndim = 0
    assert gpu.lib.pyas_wcomoments_combine_grid(gpu.handle, 8, ctypes.byref(g), 8, None) == _lib.ENOTSUP
    assert gpu.lib.pyas_wcomoments_combine_segments(gpu.handle, None, None, None, 1, None, None) == _lib.EINVAL
