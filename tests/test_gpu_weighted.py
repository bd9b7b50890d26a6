"""``Active.mean`` / ``Active.sum`` with ``weights=`` on the device against a
NumPy oracle: the selection is taken with NumPy, masked with
``oracle.storage_ref.mask_missing`` and converted with ``astype(float64)``;
``W`` is the outer product of the weight vectors taken at the selected global
indices, masked like the data; ``num = (W x).sum``, ``den = W.sum``.

Tolerance (derived, not measured).  Both sides are f64 sums of the same terms
in different orders, ``u = 2^-53`` per operation.  For each output, with
``n_sel`` the number of selected elements reduced into it:
``|got - want| <= 4 (n_sel + 8) 2^-53 sum(w |x|) / sum(w)`` for a mean, the
same without the division for a sum.  Masks, ``n`` and the positions with
``sum(w) == 0`` are exact; the dtype is float64; NaN where the oracle has NaN.
(Each check prints its largest error as a fraction of the bound; on an MI355X
the largest over this file was 0.11.)
"""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import weighted
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


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


def _per_dim(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    if Ellipsis in index:
        k = index.index(Ellipsis)
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def oracle(data, attrs, index, axis, weights, missing=None):
    """``(num, den, n, bound_num, n_sel)`` with ``keepdims`` shapes: the sums
    over the unmasked selected elements, the sum of ``w |x|`` the tolerance is
    relative to, and the number of selected elements per output."""
    sel = np.ma.asarray(ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {})))
    ok = ~np.ma.getmaskarray(sel)
    with np.errstate(all="ignore"):
        x = np.where(ok, np.ma.getdata(sel).astype(np.float64), 0.0)
    nd = data.ndim
    W = np.ones(sel.shape)
    for d, ix in enumerate(_per_dim(index, nd)):          # ascending dimension order
        if d in weights:
            w = np.asarray(weights[d], np.float64)[np.arange(data.shape[d])[ix]]
            W = W * w.reshape([-1 if k == d else 1 for k in range(nd)])
    W = np.where(ok, W, 0.0)
    axis = tuple(range(nd)) if axis is None else axis
    with np.errstate(all="ignore"):
        num = (W * x).sum(axis=axis, keepdims=True)
        den = W.sum(axis=axis, keepdims=True)
        mag = (W * np.abs(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0))).sum(axis=axis, keepdims=True)
    n = ok.sum(axis=axis, keepdims=True)
    n_sel = int(np.prod([sel.shape[a] for a in axis]))
    return num, den, n, mag, n_sel


def check(got, want, method, what=""):
    num, den, n, mag, n_sel = want
    assert isinstance(got, np.ma.MaskedArray), what
    assert got.dtype == np.float64 and got.shape == num.shape, (what, got.shape, num.shape)
    wm = (den == 0) if method == "mean" else (n == 0)
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    with np.errstate(all="ignore"):
        w = (num / den if method == "mean" else num)[~wm]
        bound = 4 * (n_sel + 8) * U * (mag / den if method == "mean" else mag)[~wm]
    g = got.data[~wm]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    err = np.abs(g[~nan] - w[~nan])
    with np.errstate(all="ignore"):
        frac = np.where(bound[~nan] > 0, err / bound[~nan], np.where(err == 0, 0.0, np.inf))
    print(what, method, "max error / bound", frac.max() if frac.size else 0.0)
    assert (err <= bound[~nan]).all(), (what, float(frac.max()))


def query(var, method, axis, weights, index, **kw):
    a = Active(var, **kw)
    getattr(a, method)(axis=axis, weights=weights)
    return a[index]


def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8"]
INDEXES = [
    ("all", (Ellipsis,)),
    ("inner", (slice(1, -1), slice(1, -1), slice(1, -1))),
    ("stride", (slice(None), slice(None, None, 3), slice(None))),
    ("list", (slice(None), [0, 5, 6, 21], slice(None))),
    # [::-2, :, 3:30]: the planner takes slices of step >= 1 only, so Active gets the same positions as an
    # index list; test_negative_step_in_a_chunk runs the slice itself
    ("neg", (list(range(14, -1, -2)), slice(None), slice(3, 30))),
]
AXES = [None, (0,), (1,), (2,), (0, 2)]
WSETS = [(1,), (0, 1, 2), (2,), (0, 2)]


@functools.lru_cache(maxsize=None)
def sweep_weights():
    """Positive weights per dim; dim 1's are exactly 0 at its first and last
    index, so kept rows there come out masked through ``sum(w) == 0``."""
    rng = np.random.default_rng(900)
    w = [rng.uniform(0.25, 2.0, n) for n in SHAPE]
    w[1] = np.cos(np.linspace(-np.pi / 2, np.pi / 2, SHAPE[1]))
    w[1][0] = w[1][-1] = 0.0
    assert (w[1][1:-1] > 0).all()
    return w


def wset(dims, shape=SHAPE):
    w = sweep_weights()
    assert shape == SHAPE
    return {d: w[d] for d in dims}


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked):
    dt = np.dtype(dt)
    rng = np.random.default_rng(100 + DTYPES.index(dt.str if dt.str in DTYPES else "|u1"))
    if dt.kind == "f":
        data = rng.normal(288.0, 10.0, SHAPE).astype(dt)
        fill, lo, hi = -999.0, 200.0, 380.0
    elif dt == np.dtype("<i8"):
        # odd values up to 2^56 in magnitude: most lie beyond 2^53 and round to nearest on conversion
        data = (rng.integers(-2 ** 55, 2 ** 55, SHAPE) * 2 + 1).astype(dt)
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 60), 2 ** 60
    elif dt == np.dtype("|u1"):
        data = rng.integers(10, 240, SHAPE).astype(dt)
        fill, lo, hi = 255, 5, 250
    else:
        data = rng.integers(-3000, 3000, SHAPE).astype(dt)
        fill, lo, hi = -32768, -3100, 3100
    attrs = {}
    if masked:
        flat = data.reshape(-1)
        flat[rng.choice(flat.size, flat.size // 50, replace=False)] = fill   # 2 %
        outl = rng.choice(flat.size, 40, replace=False)
        if dt.kind == "f" or dt == np.dtype("<i2"):   # a few beyond valid_min / valid_max
            flat[outl[:20]] = dt.type(lo - 50)
            flat[outl[20:]] = dt.type(hi + 50)
        one = lambda v: np.array([v], dtype=dt.newbyteorder("="))
        attrs = {"_FillValue": one(fill), "valid_min": one(lo), "valid_max": one(hi)}
    return data, attrs, make_var(data, CHUNKS, attrs, pad=fill)


def _sweep_cases():
    k = 0
    for dt, (iname, index), axis, masked in itertools.product(DTYPES, INDEXES, AXES, (False, True)):
        dims, method = WSETS[k % 4], ("mean", "sum")[(k // 4) % 2]   # weight sets and mean / sum rotate
        k += 1
        yield pytest.param(dt, index, axis, masked, dims, method,
                           id=f"{dt[1:]}-{iname}-{'all' if axis is None else ''.join(map(str, axis))}-"
                              f"{'masked' if masked else 'plain'}-w{''.join(map(str, dims))}-{method}")


@pytest.mark.parametrize("dt,index,axis,masked,dims,method", list(_sweep_cases()))
def test_sweep(gpu, dt, index, axis, masked, dims, method):
    data, attrs, var = sweep_var(dt, masked)
    got = query(var, method, axis, wset(dims), index)
    check(got, oracle(data, attrs, index, axis, wset(dims)), method)


def test_sweep_masks_rows_of_zero_weight(gpu):
    """Kept rows whose every weight is exactly 0 are masked in a mean (and 0,
    unmasked, in a sum)."""
    data, attrs, var = sweep_var("<f4", False)
    mean = query(var, "mean", (0, 2), wset((1,)), Ellipsis)
    assert np.ma.getmaskarray(mean)[0, :, 0].tolist() == [True] + [False] * 20 + [True]
    total = query(var, "sum", (0, 2), wset((1,)), Ellipsis)
    assert not np.ma.getmaskarray(total).any() and total.data[0, 0, 0] == 0.0 and total.data[0, 21, 0] == 0.0


# -- 2. vector edges and shuffle -----------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_var(which, dt="<f4"):
    rng = np.random.default_rng(7)
    if which == "one":      # a single chunk, innermost 31: 16-byte vectors straddle rows
        data = rng.normal(288.0, 10.0, (33, 65, 31)).astype(dt)
        return data, make_var(data, data.shape)
    if which == "short":    # innermost extent shorter than a vector of 16 u1: the per-element walk
        data = rng.integers(0, 255, (9, 11, 5)).astype(dt)
        return data, make_var(data, data.shape)
    data = rng.normal(288.0, 10.0, (64, 64, 16)).astype(dt)
    return data, make_var(data, (32, 64, 16), shuffle=(which == "shuffled"))


def edge_weights(shape):
    rng = np.random.default_rng(8)
    return {d: rng.uniform(0.1, 3.0, n) for d, n in enumerate(shape)}


@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None), slice(None), slice(None))], ids=["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
@pytest.mark.parametrize("which,dt", [("one", "<f4"), ("two", "<f4"), ("shuffled", "<f4"), ("shuffled", "<f8"),
                                      ("short", "|u1")])
def test_vector_edges_and_shuffle(gpu, which, dt, axis, index):
    data, var = edge_var(which, dt)
    w = edge_weights(data.shape)
    for method in ("mean", "sum"):
        check(query(var, method, axis, w, index), oracle(data, None, index, axis, w), method)


# -- 2b. other ranks, and factors beyond the LDS cap ------------------------------
# The full reduction keeps a chunk's factors in LDS for rank <= 3 and at most
# 2,048 factors (rank 1 and 2 with leading padding digits) and reads them from
# the pool otherwise (8 position digits): rank 4, and rows longer than the cap.
RANK_CASES = {
    "4d": ((5, 6, 7, 33), (3, 4, 4, 20), (1, 3)),       # rank 4: the global-memory run; edge chunks walk
    "4d-one": ((3, 4, 5, 31), (3, 4, 5, 31), (0, 2)),   # rank 4, one chunk, vectors straddle rows
    "2d": ((37, 45), (20, 31), (1,)),                   # rank 2 in LDS (one padding digit)
    "2d-long": ((3, 2501), (3, 2501), (1,)),            # 2,504 factors: the pool, rows of 2,501 straddle
    "1d": ((1000,), (300,), None),                      # rank 1 in LDS (two padding digits)
    "1d-long": ((5003,), (5003,), None),                # rank 1, 5,003 factors: the pool
}


@functools.lru_cache(maxsize=None)
def rank_var(name, masked):
    shape, chunks, _ = RANK_CASES[name]
    rng = np.random.default_rng(60 + sorted(RANK_CASES).index(name))
    data = rng.normal(288.0, 10.0, shape).astype("<f4")
    attrs = {}
    if masked:
        flat = data.reshape(-1)
        flat[rng.choice(flat.size, max(flat.size // 50, 1), replace=False)] = -999.0
        flat[rng.choice(flat.size, 3, replace=False)] = 500.0
        attrs = {"_FillValue": np.array([-999.0], "<f4"), "valid_min": np.array([200.0], "<f4"),
                 "valid_max": np.array([380.0], "<f4")}
    weights = {d: rng.uniform(0.1, 3.0, n) for d, n in enumerate(shape)}
    return data, attrs, make_var(data, chunks, attrs, pad=-999.0), weights


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None),)], ids=["whole", "from1"])
@pytest.mark.parametrize("name", sorted(RANK_CASES))
def test_ranks_and_long_rows(gpu, name, index, masked):
    data, attrs, var, w = rank_var(name, masked)
    for axis in (None, RANK_CASES[name][2]):
        for method in ("mean", "sum"):
            check(query(var, method, axis, w, index), oracle(data, attrs, index, axis, w), method,
                  f"{name} {axis}")


# -- 3. tiles --------------------------------------------------------------------
def test_small_tiles_merge_in_order(gpu):
    """More than one tile per chunk (and tile boundaries inside rows): within
    the bound, and the same bytes when repeated."""
    data, var = edge_var("one")
    w = edge_weights(data.shape)
    cut = (slice(1, None),)
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        got = [query(var, "mean", None, w, (Ellipsis,)) for _ in range(2)]
        part = [query(var, "sum", None, w, cut) for _ in range(2)]
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)
    check(got[0], oracle(data, None, (Ellipsis,), None, w), "mean")
    check(part[0], oracle(data, None, cut, None, w), "sum")
    assert _bytes(got[0]) == _bytes(got[1]) and _bytes(part[0]) == _bytes(part[1])


# -- 4. determinism and residency ---------------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_deterministic_and_resident(gpu, axis):
    data, attrs, var = sweep_var("<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))
    w = wset((0, 1, 2))
    first = query(var, "mean", axis, w, index)
    assert _bytes(query(var, "mean", axis, w, index)) == _bytes(first)
    plain = Active(var, axis=axis).mean()[index]
    try:
        r = Active(var, axis=axis, resident=True)
        assert _bytes(r.mean(weights=w)[index]) == _bytes(first)
        assert _bytes(r.mean()[index]) == _bytes(plain)            # weights are per query
        assert _bytes(r.mean()[index]) == _bytes(plain)            # the cached replay
        assert _bytes(r.mean(weights=w)[index]) == _bytes(first)   # weighted after a cached plain mean
        assert _bytes(r.sum(weights=w)[index]) == _bytes(query(var, "sum", axis, w, index))
    finally:
        release_resident(var)


def test_unweighted_queries_unchanged(gpu):
    """A query without weights returns the bytes (and dtype) it did before,
    also right after a weighted one on the same object."""
    data, attrs, var = sweep_var("<i2", True)
    a = Active(var, axis=(1,))
    want_mean, want_sum = a.mean()[1:-1], a.sum()[1:-1]
    a.mean(weights=wset((1,)))[1:-1]
    got_mean, got_sum = a.mean()[1:-1], a.sum()[1:-1]
    assert got_mean.dtype == want_mean.dtype and _bytes(got_mean) == _bytes(want_mean)
    assert got_sum.dtype == want_sum.dtype and _bytes(got_sum) == _bytes(want_sum)


# -- 5. select, not multiply ---------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_masked_values_never_reach_a_product(gpu, axis):
    rng = np.random.default_rng(51)
    data = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    data[1, 2, 3] = np.inf                      # masked by valid_max
    data[6, 9, 7] = 1e30                        # the fill value
    data[3, 3, 3] = 1e30
    attrs = {"_FillValue": np.array([1e30], "<f4"), "valid_max": np.array([1e6], "<f4")}
    var = make_var(data, (4, 6, 5), attrs)
    w = {0: rng.uniform(0.5, 2.0, 8), 2: rng.uniform(0.5, 2.0, 10)}
    for method in ("mean", "sum"):
        got = query(var, method, axis, w, Ellipsis)
        assert np.isfinite(got.data).all() and not np.ma.getmaskarray(got).any()
        check(got, oracle(data, attrs, Ellipsis, axis, w), method)


def test_unmasked_nan_gives_nan(gpu):
    rng = np.random.default_rng(52)
    data = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    data[1, 2, 3] = np.nan
    var = make_var(data, (4, 6, 5))
    w = {1: rng.uniform(0.5, 2.0, 12)}
    for axis, n_nan in ((None, 1), ((0,), 1), ((2,), 1), ((0, 2), 1)):
        for method in ("mean", "sum"):
            got = query(var, method, axis, w, Ellipsis)
            assert np.isnan(got.data).sum() == n_nan
            check(got, oracle(data, None, Ellipsis, axis, w), method)


# -- 6. all-ones weights ------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (1,), (0, 2)], ids=["all", "1", "02"])
def test_all_ones_weights_equal_plain_mean_and_sum(gpu, axis):
    data, attrs, var = sweep_var("<f4", True)
    ones = {d: np.ones(n) for d, n in enumerate(SHAPE)}
    index = (slice(1, -1), slice(None), slice(2, 35))
    sel = ref.mask_missing(data[index], get_missing_attributes(attrs)).astype(np.float64)
    want = oracle(data, attrs, index, axis, ones)
    for method, fn in (("mean", np.ma.mean), ("sum", np.ma.sum)):
        got = query(var, method, axis, ones, index)
        check(got, want, method)
        ref_val = fn(sel, axis=axis, keepdims=True)
        assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(ref_val))
        bound = 4 * (want[4] + 8) * U * (want[3] / want[1] if method == "mean" else want[3])
        assert (np.abs(got.data - np.ma.getdata(ref_val)) <= bound)[~np.ma.getmaskarray(got)].all()
    a = Active(var, axis=axis)
    a.components = True
    n = a.mean(weights=ones)[index]["n"]
    a = Active(var, axis=axis)
    a.components = True
    plain = a.mean()[index]["n"]
    assert np.ma.getdata(n).tobytes() == np.ma.getdata(plain).astype(np.int64).tobytes()
    np.testing.assert_array_equal(np.ma.getdata(n), sel.count(axis=axis, keepdims=True))


# -- 7. components -----------------------------------------------------------------
def test_components(gpu):
    rng = np.random.default_rng(31)
    data = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    data[:, 7, 3] = -999.0                # one axis-0 output entirely masked
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    var = make_var(data, (4, 6, 5), attrs)
    w = {0: rng.uniform(0.5, 2.0, 8), 1: rng.uniform(0.0, 2.0, 12)}
    w[1][2] = 0.0                         # unmasked elements of weight exactly 0
    num, den, n, mag, n_sel = oracle(data, attrs, Ellipsis, (0,), w)
    for method, keys in (("mean", ["n", "sum", "sum_of_weights"]), ("sum", ["n", "sum"])):
        a = Active(var, axis=(0,))
        a.components = True
        got = getattr(a, method)(weights=w)[...]
        assert sorted(got) == keys
        assert got["n"].dtype == np.int64 and got["sum"].dtype == np.float64
        assert not np.ma.getmaskarray(got["n"]).any()
        np.testing.assert_array_equal(np.ma.getdata(got["n"]), n)
        empty = n == 0
        assert empty[0, 7, 3] and empty.sum() == 1
        assert np.array_equal(np.ma.getmaskarray(got["sum"]), empty)     # masked where n == 0, not where sw == 0
        bound = 4 * (n_sel + 8) * U * mag
        assert (np.abs(np.ma.getdata(got["sum"]) - num) <= bound).all()
        if method == "mean":
            assert got["sum_of_weights"].dtype == np.float64
            assert np.array_equal(np.ma.getmaskarray(got["sum_of_weights"]), empty)
            assert (np.abs(np.ma.getdata(got["sum_of_weights"]) - den) <= 4 * (n_sel + 8) * U * den).all()
            assert (np.ma.getdata(got["sum_of_weights"])[0, 2, :] == 0.0).all()
            rec = weighted.records(np.ma.getdata(got["n"]), np.ma.getdata(got["sum_of_weights"]),
                                   np.ma.getdata(got["sum"]))
            assert _bytes(weighted.finalize(rec)) == _bytes(query(var, "mean", (0,), w, Ellipsis))


# -- 8. a netCDF file -----------------------------------------------------------------
NC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nc")


@pytest.mark.parametrize("axis", [None, (0,), (1, 2)], ids=["all", "0", "12"])
def test_netcdf_file_cos_weights(gpu, axis):
    """tas of test1.nc by file path and as a ChunkedVariable, cos-shaped
    weights on dimension 1; the data come from the method=None selection."""
    from tests.test_gpu_active import variable
    path, key = os.path.join(NC, "test1.nc"), "test1.nc:tas"
    sel = np.ma.asarray(Active(path, "tas")[...])
    shape = sel.shape
    w = {1: np.cos(np.linspace(-np.pi / 2, np.pi / 2, shape[1] + 2))[1:-1]}
    index = tuple(slice(n // 4, n) for n in shape)
    data = np.ma.getdata(sel)
    # (mask_missing in the oracle masks from the variable's attributes again)
    attrs = variable(key).attrs
    assert np.array_equal(np.ma.getmaskarray(ref.mask_missing(data, get_missing_attributes(attrs))),
                          np.ma.getmaskarray(sel))
    for method in ("mean", "sum"):
        want = oracle(data, attrs, index, axis, w)
        by_path = query(path, method, axis, w, index, ncvar="tas")
        by_var = query(variable(key), method, axis, w, index)
        check(by_path, want, method)
        assert _bytes(by_var) == _bytes(by_path)


# -- 9. vector _FillValue ---------------------------------------------------------------
def test_vector_fill_value(gpu):
    """A vector ``_FillValue`` (broadcast over the last dim of each chunk's
    selection) takes the per-chunk selections and host-built segments."""
    rng = np.random.default_rng(41)
    data = rng.normal(10.0, 3.0, (8, 6, 10)).astype("<f4")
    vec = np.array([1.0, 2.0, 3.0, 4.0, 5.0], "<f4")
    hit = rng.random(data.shape) < 0.1
    data[hit] = np.broadcast_to(np.tile(vec, 2), data.shape)[hit]
    var = make_var(data, (4, 3, 5), {"_FillValue": vec})
    missing = (np.tile(vec, 2), None, None, None)      # the same rule over the whole selection
    w = {0: rng.uniform(0.5, 2.0, 8), 2: rng.uniform(0.5, 2.0, 10)}
    for axis in (None, (0,), (2,)):
        for method in ("mean", "sum"):
            check(query(var, method, axis, w, Ellipsis), oracle(data, None, Ellipsis, axis, w, missing=missing),
                  method, f"{axis}")


# -- 10. the C entry point ---------------------------------------------------------------
@pytest.mark.parametrize("axes", [(0, 1, 2), (0,), (2,), (0, 2)], ids=["all", "0", "2", "02"])
def test_negative_step_in_a_chunk(gpu, axes):
    """``chunk[::-2, :, 3:30]`` of one (15, 22, 37) chunk through
    pyas_wsum_axes itself (negative steps exist below the planner)."""
    from pyactivestorage_amd import engine, selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    data, attrs, _ = sweep_var("<f4", True)
    index = (slice(None, None, -2), slice(None), slice(3, 30))
    w = wset((0, 1, 2))
    st = gpu.thread_stream()
    buf = DeviceBuffer(gpu, data.nbytes)
    gpu.h2d(buf.ptr, np.ascontiguousarray(data), st)
    plan = ReductionPlan(gpu, data.dtype, data.shape, buf.ptr, np.zeros(1, np.int64),
                         selections=[selection.normalize(index, data.shape)],
                         missing=get_missing_attributes(attrs), stream=st)
    want = oracle(data, attrs, index, axes, w)
    out = np.zeros(want[0].size, engine.wsum_dtype)
    pool = np.concatenate([w[0], w[1], w[2]])
    origin = np.zeros((1, 8), np.int32)
    origin[0, :3] = (0, SHAPE[0], SHAPE[0] + SHAPE[1])
    obuf, off = DeviceBuffer(gpu, out.nbytes), DeviceBuffer(gpu, 16)
    wbuf, gbuf = DeviceBuffer(gpu, pool.nbytes), DeviceBuffer(gpu, origin.nbytes)
    gpu.h2d(off.ptr, np.zeros(1, np.int64), st)
    gpu.h2d(wbuf.ptr, pool, st)
    gpu.h2d(gbuf.ptr, origin, st)
    mask = 0
    for a in axes:
        mask |= 1 << a
    engine.wsum_axes(gpu, plan.batch, plan.mask_up.struct, wbuf.ptr, gbuf.ptr, mask, off.ptr, obuf.ptr, st)
    gpu.d2h(out, obuf.ptr, st)
    gpu.synchronize(st)
    out = out.reshape(want[0].shape)
    np.testing.assert_array_equal(out["count"], want[2])
    check(weighted.finalize(out), want, "mean")
    check(weighted.finalize(out, mean=False), want, "sum")


def test_entry_point_errors(gpu):
    from pyactivestorage_amd import _lib
    b = _lib.Batch()
    b.dtype, b.ndim, b.n_chunks = _lib.F32, 9, 0
    m, w = _lib.Mask(), _lib.Weights()
    call = lambda axes: gpu.lib.pyas_wsum_axes(gpu.handle, ctypes.byref(b), ctypes.byref(m), ctypes.byref(w), axes,
                                               None, None, None)
    assert call(1) == _lib.ENOTSUP
    b.ndim = 2
    b.chunk_shape[0] = b.chunk_shape[1] = 4
    assert call(4) == _lib.EINVAL
    b.n_chunks = 1                      # a chunk, but no data / weights
    assert call(3) == _lib.EINVAL
    g = _lib.Grid()
    g.ndim = 0
    assert gpu.lib.pyas_wsum_combine_grid(gpu.handle, 8, ctypes.byref(g), 8, None) == _lib.ENOTSUP
    assert gpu.lib.pyas_wsum_combine_segments(gpu.handle, None, None, None, 1, None, None) == _lib.EINVAL


# -- 11. group= ------------------------------------------------------------------------
def test_group_with_weights_not_implemented(gpu):
    data, attrs, var = sweep_var("<f4", False)
    for method in ("mean", "sum"):
        a = Active(var, group=object())
        with pytest.raises(NotImplementedError, match="weights with group="):
            getattr(a, method)(weights=wset((1,)))[...]


# -- 12. branches the shapes above do not reach (the cases of tests/_stats_gaps.py) -----------
from tests import _stats_gaps as G   # noqa: E402

MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


@functools.lru_cache(maxsize=None)
def gap_var(group, name, dt="<f4", masked=False, shuffle=None):
    data, attrs = G.single(group, name, dt, masked)
    _, chunks, _, _, shuffled = G.case(group, name)
    shuffle = shuffled if shuffle is None else shuffle
    return data, attrs, make_var(data, chunks, attrs, shuffle=shuffle, pad=G.fill_of(attrs, dt))


def gap_check(group, name, dt, masked, iname, axis, shuffle=None, dims=None):
    data, attrs, var = gap_var(group, name, dt, masked, shuffle)
    index = G.index_of(group, name, iname)
    w = G.weights(data.shape, dims)
    want = oracle(data, attrs, index, axis, w)
    for method in ("mean", "sum"):
        check(query(var, method, axis, w, index), want, method, f"{group} {name} {dt} {iname} {G.axis_id(axis)}")


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(gpu, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in its launch."""
    data, attrs, var = gap_var("G2", name, "<f4", masked)
    k = G.G2_SECOND_TRIP
    w = G.weights(data.shape)
    want = oracle(data, attrs, Ellipsis, (0,), w)
    tail = tuple(v.reshape(-1)[k:] for v in want[:4]) + (want[4],)
    for method in ("mean", "sum"):
        got = query(var, method, (0,), w, Ellipsis)
        assert got.shape == (1, 130, 130)
        check(got.reshape(-1)[k:], tail, method, f"G2 {name}: the second trip, outputs {k}..16899")
        check(got, want, method, f"G2 {name}: every output")


@MASKED
@pytest.mark.parametrize("iname", ["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=G.axis_id)
@pytest.mark.parametrize("dt", G.G3_DTYPES)
@pytest.mark.parametrize("name", ["odd", "odd17"])
def test_g3_shuffled_chunks_of_odd_size(gpu, name, dt, axis, iname, masked):
    """Shuffled chunks of 105 elements (rows of 7: the full reduction walks)
    and of 255 (rows of 17: ws_run_shuffled's per-element fallback)."""
    gap_check("G3", name, dt, masked, iname, axis)


@pytest.mark.parametrize("iname", list(G.G3_RUNS))
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_runs_inside_a_shuffled_chunk(gpu, dt, iname):
    gap_check("G3", "runs", dt, False, iname, None)


@MASKED
def test_g4_rank_8(gpu, masked):
    """PYAS_MAX_DIMS dims, weight vectors on the first and the last."""
    for iname, _, axis, _ in G.combos("G4", "8d"):
        gap_check("G4", "8d", "<f4", masked, iname, axis, dims=(0, 7))


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    for axis in (None, (1,)):
        gap_check("G5", "dtypes", dt, masked, "whole", axis, shuffle)


@pytest.mark.parametrize("dt,off", G.G6_CASES)
def test_g6_base_misaligned(gpu, dt, off):
    """One chunk ``off`` bytes into its buffer, every dim reduced, through
    pyas_wsum_axes itself: the head and tail of ws_run_plain, and the position
    its vectors' weights start from."""
    from pyactivestorage_amd import engine
    from pyactivestorage_amd.device import DeviceBuffer
    data = G.g6_chunk(dt)
    w = G.weights(data.shape)
    pool = np.concatenate([w[0], w[1], w[2]])
    origin = np.zeros((1, 8), np.int32)
    origin[0, :3] = (0, data.shape[0], data.shape[0] + data.shape[1])
    for iname, index in G.G6_INDEXES.items():
        st, buf, plan = G.misaligned_plan(gpu, data, off, index)
        out = np.zeros(1, engine.wsum_dtype)
        obuf, zero = DeviceBuffer(gpu, out.nbytes), DeviceBuffer(gpu, 16)
        wbuf, gbuf = DeviceBuffer(gpu, pool.nbytes), DeviceBuffer(gpu, origin.nbytes)
        gpu.h2d(zero.ptr, np.zeros(1, np.int64), st)
        gpu.h2d(wbuf.ptr, pool, st)
        gpu.h2d(gbuf.ptr, origin, st)
        engine.wsum_axes(gpu, plan.batch, plan.mask_up.struct, wbuf.ptr, gbuf.ptr, 0b111, zero.ptr, obuf.ptr, st)
        gpu.d2h(out, obuf.ptr, st)
        gpu.synchronize(st)
        want = oracle(data, None, Ellipsis if index is None else index, None, w)
        out = out.reshape(1, 1, 1)
        np.testing.assert_array_equal(out["count"], want[2])
        check(weighted.finalize(out), want, "mean", f"G6 {dt} offset {off} {iname}")
        check(weighted.finalize(out, mean=False), want, "sum", f"G6 {dt} offset {off} {iname}")
