"""``Active.var`` / ``Active.std`` on the device against ``np.ma.var`` /
``np.ma.std`` of the float64 copy of the masked selection (the selection is
taken with NumPy and masked with ``oracle.storage_ref.mask_missing``).

Tolerance: 1e-9 relative on the value, ``var`` and ``std`` alike; mask and
count exact; dtype float64; NaN where the oracle has NaN.  Every accumulated
term ``(x-K)^2`` is non-negative, so a lane's sum is off by at most about
``n_lane * 2^-53``; the ``s1^2/n`` correction is amplified by at most
``1 + (K-mu)^2/sigma^2`` with K a data value, within 6 sigma here; a lane sees
at most 2^18/256 elements: about 1e-11 in all.  ``sum x^2 - (sum x)^2/n``
misses 1e-9 by four orders of magnitude on the offset case below.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import moments
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

RTOL = 1e-9


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


def oracle(data, attrs, index, axis, method, ddof, missing=None):
    sel = ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {}))
    fn = np.ma.var if method == "var" else np.ma.std
    with np.errstate(all="ignore"):
        return fn(sel.astype(np.float64), axis=axis, ddof=ddof, keepdims=True)


def check(got, want, what=""):
    assert isinstance(got, np.ma.MaskedArray), what
    assert got.dtype == np.float64 and got.shape == np.shape(want), (what, got.shape, np.shape(want))
    wm = np.ma.getmaskarray(want)
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    g, w = got.data[~wm], np.ma.getdata(want)[~wm]
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(g), nan), what
    err = np.abs(g[~nan] - w[~nan]) / np.where(w[~nan] == 0, 1.0, np.abs(w[~nan]))
    print(what, "max relative error", err.max() if err.size else 0.0)
    np.testing.assert_allclose(g[~nan], w[~nan], rtol=RTOL, atol=0, err_msg=what)


def query(var, method, axis, ddof, index, **kw):
    a = Active(var, **kw)
    getattr(a, method)(axis=axis, ddof=ddof)
    return a[index]


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8"]
INDEXES = [
    ("all", (Ellipsis,)),
    ("inner", (slice(1, -1), slice(1, -1), slice(1, -1))),
    ("stride", (slice(None), slice(None, None, 3), slice(None))),
    ("list", (slice(None), [0, 5, 6, 21], slice(None))),
    # [::-2, :, 3:30]: the planner takes slices of step >= 1 only (IndexError for every method), so
    # Active gets the same positions as an index list; test_negative_step_in_a_chunk runs the slice itself
    ("neg", (list(range(14, -1, -2)), slice(None), slice(3, 30))),
]
NUMPY_INDEX = {"neg": (slice(None, None, -2), slice(None), slice(3, 30))}
AXES = [None, (0,), (1,), (2,), (0, 2)]
MOMENTS = [("var", 0), ("var", 1), ("std", 0), ("std", 1)]


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked):
    dt = np.dtype(dt)
    rng = np.random.default_rng(100 + DTYPES.index(dt.str if dt.str in DTYPES else "|u1"))
    if dt.kind == "f":
        data = rng.normal(288.0, 10.0, SHAPE).astype(dt)
        fill, lo, hi = -999.0, 200.0, 380.0
    elif dt == np.dtype("<i8"):
        # Odd values up to 2^56 in magnitude: most lie beyond 2^53 and round to nearest on
        # conversion.  They are spread about zero, not offset: a record carries its mean as one
        # f64, so merging records costs about 2^-53 |mean| / sigma (pyas.h), which an offset of
        # 2^53 under a spread of 2^32 would put at 1e-9 for outputs of a few elements.
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
        method, ddof = MOMENTS[k % 4]   # every dtype / index / axes / mask once; the four moments rotate
        k += 1
        yield pytest.param(dt, iname, index, axis, masked, method, ddof,
                           id=f"{dt[1:]}-{iname}-{'all' if axis is None else ''.join(map(str, axis))}-"
                              f"{'masked' if masked else 'plain'}-{method}{ddof}")


@pytest.mark.parametrize("dt,iname,index,axis,masked,method,ddof", list(_sweep_cases()))
def test_sweep(gpu, dt, iname, index, axis, masked, method, ddof):
    data, attrs, var = sweep_var(dt, masked)
    got = query(var, method, axis, ddof, index)
    check(got, oracle(data, attrs, NUMPY_INDEX.get(iname, index), axis, method, ddof))


@pytest.mark.parametrize("axes", [(0, 1, 2), (0,), (2,), (0, 2)], ids=["all", "0", "2", "02"])
def test_negative_step_in_a_chunk(gpu, axes):
    """``chunk[::-2, :, 3:30]`` of one (15, 22, 37) chunk through
    pyas_moments_axes itself (negative steps exist below the planner)."""
    from pyactivestorage_amd import _lib, engine, selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    data, attrs, _ = sweep_var("<f4", True)
    index = NUMPY_INDEX["neg"]
    st = gpu.thread_stream()
    buf = DeviceBuffer(gpu, data.nbytes)
    gpu.h2d(buf.ptr, np.ascontiguousarray(data), st)
    plan = ReductionPlan(gpu, data.dtype, data.shape, buf.ptr, np.zeros(1, np.int64),
                         selections=[selection.normalize(index, data.shape)],
                         missing=get_missing_attributes(attrs), stream=st)
    want = oracle(data, attrs, index, axes, "var", 0)
    out = np.zeros(want.size, engine.moments_dtype)
    obuf, off = DeviceBuffer(gpu, out.nbytes), DeviceBuffer(gpu, 16)
    gpu.h2d(off.ptr, np.zeros(1, np.int64), st)
    mask = 0
    for a in axes:
        mask |= 1 << a
    engine.moments_axes(gpu, plan.batch, plan.mask_up.struct, mask, off.ptr, obuf.ptr, st)
    gpu.d2h(out, obuf.ptr, st)
    gpu.synchronize(st)
    check(moments.finalize(out.reshape(want.shape)), want)


# -- 2. vector-load edges, 3. shuffled bytes ----------------------------------
@functools.lru_cache(maxsize=None)
def edge_var(which, dt="<f4"):
    rng = np.random.default_rng(7)
    if which == "one":      # a single chunk: unroll step, 16-byte head and tail, tile merge
        data = rng.normal(288.0, 10.0, (33, 65, 31)).astype(dt)
        return data, make_var(data, data.shape)
    data = rng.normal(288.0, 10.0, (64, 64, 16)).astype(dt)
    return data, make_var(data, (32, 64, 16), shuffle=(which == "shuffled"))


@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, None), slice(None), slice(None))], ids=["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
@pytest.mark.parametrize("which,dt", [("one", "<f4"), ("two", "<f4"), ("shuffled", "<f4"), ("shuffled", "<f8")])
def test_vector_edges_and_shuffle(gpu, which, dt, axis, index):
    data, var = edge_var(which, dt)
    for method, ddof in (("var", 0), ("std", 1)):
        check(query(var, method, axis, ddof, index), oracle(data, None, index, axis, method, ddof))


def test_small_tiles_merge_in_order(gpu):
    """More than one tile per chunk (and a tile boundary inside the run)."""
    data, var = edge_var("one")
    want = oracle(data, None, (Ellipsis,), None, "var", 0)
    base = query(var, "var", None, 0, (Ellipsis,))
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        got = query(var, "var", None, 0, (Ellipsis,))
        cut = query(var, "var", None, 0, (slice(1, None),))
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)
    check(got, want)
    check(base, want)
    check(cut, oracle(data, None, (slice(1, None),), None, "var", 0))


# -- 4. conditioning -----------------------------------------------------------
def test_constant_field_is_exactly_zero(gpu):
    data = np.full((20, 30, 17), 287.65, "<f4")
    var = make_var(data, (8, 12, 20), pad=1.0)
    for axis in (None, (0,), (2,), (0, 2)):
        for method in ("var", "std"):
            got = query(var, method, axis, 0, Ellipsis)
            assert not np.ma.getmaskarray(got).any()
            assert (got.data == 0.0).all(), (axis, method, got)


@pytest.mark.parametrize("name", ["offset", "temperature"])
def test_conditioning(gpu, name):
    rng = np.random.default_rng(21)
    if name == "offset":   # sum x^2 - (sum x)^2 / n is off by 1.9e-5 relative here
        data = (1e6 + rng.uniform(0, 1, (32, 32, 32))).astype("<f4")
    else:
        data = rng.normal(288.0, 10.0, (32, 32, 32)).astype("<f4")
    var = make_var(data, (16, 32, 32))
    for axis in (None, (0,), (2,)):
        for method, ddof in (("var", 0), ("std", 1)):
            check(query(var, method, axis, ddof, Ellipsis), oracle(data, None, Ellipsis, axis, method, ddof),
                  f"{name} {axis} {method}")


# -- 5. masked edge cases --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def masked_var():
    rng = np.random.default_rng(31)
    data = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    data[0:4, 0:6, 0:5] = -999.0          # one chunk entirely fill values
    data[:, 7, 3] = -999.0                # one axis-0 output column entirely masked
    data[:, 8, 2] = -999.0                # an output with a single valid element
    data[5, 8, 2] = 12.5
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    return data, attrs, make_var(data, (4, 6, 5), attrs)


@pytest.mark.parametrize("ddof", [0, 1])
@pytest.mark.parametrize("axis", [None, (0,), (1,), (2,), (0, 2)], ids=["all", "0", "1", "2", "02"])
def test_masked_edges(gpu, axis, ddof):
    data, attrs, var = masked_var()
    for method in ("var", "std"):
        got = query(var, method, axis, ddof, Ellipsis)
        check(got, oracle(data, attrs, Ellipsis, axis, method, ddof))
        if axis == (0,):
            m = np.ma.getmaskarray(got)
            assert m[0, 7, 3] and not m[0, 7, 2] and not m[0, 7, 4] and not m[0, 6, 3]
            if ddof == 0:
                assert not m[0, 8, 2] and got.data[0, 8, 2] == 0.0
            else:
                assert m[0, 8, 2]


def test_all_masked_selection(gpu):
    data, attrs, var = masked_var()
    index = (slice(0, 4), slice(0, 6), slice(0, 5))
    for axis in (None, (1,)):
        got = query(var, "var", axis, 0, index)
        assert np.ma.getmaskarray(got).all() and got.dtype == np.float64
        assert got.shape == ((1, 1, 1) if axis is None else (4, 1, 5))


@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_vector_missing_value(gpu, axis):
    """A vector ``missing_value`` (broadcast over the last dim of each chunk's
    selection) takes the per-chunk selections and host-built segments."""
    rng = np.random.default_rng(41)
    data = rng.normal(10.0, 3.0, (8, 6, 10)).astype("<f4")
    vec = np.array([1.0, 2.0, 3.0, 4.0, 5.0], "<f4")
    hit = rng.random(data.shape) < 0.1
    data[hit] = np.broadcast_to(np.tile(vec, 2), data.shape)[hit]
    var = make_var(data, (4, 3, 5), {"missing_value": vec})
    missing = (None, np.tile(vec, 2), None, None)      # the same rule over the whole selection
    for method, ddof in (("var", 0), ("std", 1)):
        got = query(var, method, axis, ddof, Ellipsis)
        check(got, oracle(data, None, Ellipsis, axis, method, ddof, missing=missing))


# -- 6. non-finite ----------------------------------------------------------------
def test_non_finite(gpu):
    """An unmasked NaN and an unmasked +inf (in different chunks) give NaN,
    as ``np.var([1, inf])`` does; every other output is unaffected."""
    rng = np.random.default_rng(51)
    data = rng.normal(10.0, 3.0, (8, 12, 10)).astype("<f4")
    data[1, 2, 3] = np.nan
    data[6, 9, 7] = np.inf
    var = make_var(data, (4, 6, 5))
    d64 = data.astype(np.float64)
    for method in ("var", "std"):
        fn = np.var if method == "var" else np.std
        for axis in (None, (0,), (2,), (0, 2)):
            got = query(var, method, axis, 0, Ellipsis)
            with np.errstate(all="ignore"):
                want = fn(d64, axis=axis, keepdims=True)
            assert np.isnan(want).sum() == (1 if axis is None else 2)
            check(got, np.ma.MaskedArray(want), f"{method} {axis}")


# -- 7. components -----------------------------------------------------------------
def test_components_merge(gpu):
    data, attrs, var = sweep_var("<f4", True)

    def comps(index, method="var", axis=(0,)):
        a = Active(var, axis=axis)
        a.components = True
        a.method = method
        return a[index]

    whole, lo, hi = comps(Ellipsis), comps(slice(0, 8)), comps(slice(8, None))
    assert sorted(whole) == ["m2", "mean", "n"]
    assert whole["mean"].dtype == np.float64 and whole["m2"].dtype == np.float64 and whole["n"].dtype == np.int64
    rec = lambda c: moments.records(np.ma.getdata(c["n"]), np.ma.getdata(c["mean"]), np.ma.getdata(c["m2"]))
    merged = moments.merge(rec(lo), rec(hi))
    np.testing.assert_array_equal(merged["count"], np.ma.getdata(whole["n"]))
    np.testing.assert_allclose(merged["mean"], np.ma.getdata(whole["mean"]), rtol=RTOL)
    np.testing.assert_allclose(merged["m2"], np.ma.getdata(whole["m2"]), rtol=RTOL)
    check(moments.finalize(merged, 1), oracle(data, attrs, Ellipsis, (0,), "var", 1))
    mean = comps(Ellipsis, "mean")
    assert np.ma.getdata(mean["n"]).tobytes() == np.ma.getdata(whole["n"]).tobytes()
    assert not np.ma.getmaskarray(whole["n"]).any()
    assert np.array_equal(np.ma.getmaskarray(whole["mean"]), np.ma.getdata(whole["n"]) == 0)


# -- 8. determinism and residency ----------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
def test_deterministic_and_resident(gpu, axis):
    from pyactivestorage_amd.active import release_resident
    data, attrs, var = sweep_var("<f4", True)
    index = (slice(1, -1), slice(None), slice(2, 35))
    first = query(var, "var", axis, 0, index)
    assert _bytes(query(var, "var", axis, 0, index)) == _bytes(first)
    fresh_mean = Active(var, axis=axis).mean()[index]
    try:
        r = Active(var, axis=axis, resident=True)
        assert _bytes(r.var()[index]) == _bytes(first)
        assert _bytes(r.mean()[index]) == _bytes(fresh_mean)     # a mean after a var
        assert _bytes(r.mean()[index]) == _bytes(fresh_mean)     # and its cached replay
        assert _bytes(r.var()[index]) == _bytes(first)           # a var after a mean
        assert _bytes(r.std(ddof=1)[index]) == _bytes(query(var, "std", axis, 1, index))
    finally:
        release_resident(var)


# -- 9. Active.sum() --------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (1,)], ids=["all", "1"])
def test_sum_method(gpu, axis):
    data, attrs, var = sweep_var("<i2", True)
    a = Active(var, axis=axis)
    a.method = "sum"
    want = a[1:-1]
    got = Active(var).sum(axis=axis)[1:-1]
    assert got.dtype == want.dtype and got.shape == want.shape and _bytes(got) == _bytes(want)


# -- the C entry points' argument checks ---------------------------------------------------
def test_entry_point_errors(gpu):
    from pyactivestorage_amd import _lib
    b = _lib.Batch()
    b.dtype, b.ndim, b.n_chunks = _lib.F32, 9, 0
    import ctypes
    m = _lib.Mask()
    assert gpu.lib.pyas_moments_axes(gpu.handle, ctypes.byref(b), ctypes.byref(m), 1, None, None, None) == _lib.ENOTSUP
    b.ndim = 2
    b.chunk_shape[0] = b.chunk_shape[1] = 4
    assert gpu.lib.pyas_moments_axes(gpu.handle, ctypes.byref(b), ctypes.byref(m), 4, None, None, None) == _lib.EINVAL
    g = _lib.Grid()
    g.ndim = 0
    assert gpu.lib.pyas_moments_combine_grid(gpu.handle, 8, ctypes.byref(g), 8, None) == _lib.ENOTSUP
    assert gpu.lib.pyas_moments_combine_segments(gpu.handle, None, None, None, 1, None, None) == _lib.EINVAL
    # a selection outside the chunk never reaches the device (the plan's bounds check)
    from pyactivestorage_amd.batch import ReductionPlan
    table = np.zeros((1, _lib.MAX_DIMS, 3), np.int32)
    table[:, :, 1:] = 1
    table[0, 0] = (2, 1, 4)
    with pytest.raises(IndexError):
        ReductionPlan(gpu, "<f4", (4, 4), 0, np.zeros(1, np.int64), sel_table=table, missing=(None,) * 4)


# -- 10. branches the shapes above do not reach (the cases of tests/_stats_gaps.py) -----------
from tests import _stats_gaps as G   # noqa: E402

BOTH = (("var", 0), ("std", 1))
MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


@functools.lru_cache(maxsize=None)
def gap_var(group, name, dt="<f4", masked=False, shuffle=None):
    data, attrs = G.single(group, name, dt, masked)
    _, chunks, _, _, shuffled = G.case(group, name)
    shuffle = shuffled if shuffle is None else shuffle
    return data, attrs, make_var(data, chunks, attrs, shuffle=shuffle, pad=G.fill_of(attrs, dt))


def gap_check(group, name, dt, masked, iname, axis, shuffle=None):
    data, attrs, var = gap_var(group, name, dt, masked, shuffle)
    index = G.index_of(group, name, iname)
    for method, ddof in BOTH:
        check(query(var, method, axis, ddof, index), oracle(data, attrs, index, axis, method, ddof),
              f"{group} {name} {dt} {iname} {G.axis_id(axis)} {method}")


@MASKED
@pytest.mark.parametrize("name,iname", [(n, i) for n in G.G1 for i in G.case("G1", n)[3]])
def test_g1_reduced_positions_beyond_the_offset_map(gpu, name, iname, masked):
    """More than kMomRoff reduced positions in a chunk: the radix-counter walk
    of k_moments_axes, a wave ("row") and a lane ("lane") per output."""
    gap_check("G1", name, "<f4", masked, iname, G.case("G1", name)[2][0])


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(gpu, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in its launch."""
    data, attrs, var = gap_var("G2", name, "<f4", masked)
    k = G.G2_SECOND_TRIP
    for method, ddof in BOTH:
        got, want = query(var, method, (0,), ddof, Ellipsis), oracle(data, attrs, Ellipsis, (0,), method, ddof)
        assert got.shape == want.shape == (1, 130, 130)
        check(got.reshape(-1)[k:], want.reshape(-1)[k:], f"G2 {name} {method}: the second trip, outputs {k}..16899")
        check(got, want, f"G2 {name} {method}: every output")


@MASKED
@pytest.mark.parametrize("iname", ["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=G.axis_id)
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_shuffled_chunks_of_odd_size(gpu, dt, axis, iname, masked):
    """Shuffled chunks of 105 elements: mom_run_shuffled's per-element fallback."""
    gap_check("G3", "odd", dt, masked, iname, axis)


@pytest.mark.parametrize("iname", list(G.G3_RUNS))
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_runs_inside_a_shuffled_chunk(gpu, dt, iname):
    gap_check("G3", "runs", dt, False, iname, None)


@MASKED
@pytest.mark.parametrize("name", list(G.G4))
def test_g4_ranks(gpu, name, masked):
    for iname, _, axis, _ in G.combos("G4", name):
        gap_check("G4", name, "<f4", masked, iname, axis)


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    for axis in (None, (1,)):
        gap_check("G5", "dtypes", dt, masked, "whole", axis, shuffle)


@pytest.mark.parametrize("dt,off", G.G6_CASES)
def test_g6_base_misaligned(gpu, dt, off):
    """One chunk ``off`` bytes into its buffer, every dim reduced, through
    pyas_moments_axes itself: the head and tail of mom_run_plain."""
    from pyactivestorage_amd import engine
    from pyactivestorage_amd.device import DeviceBuffer
    data = G.g6_chunk(dt)
    for iname, index in G.G6_INDEXES.items():
        st, buf, plan = G.misaligned_plan(gpu, data, off, index)
        out = np.zeros(1, engine.moments_dtype)
        obuf = DeviceBuffer(gpu, out.nbytes)
        engine.moments_axes(gpu, plan.batch, plan.mask_up.struct, 0b111, None, obuf.ptr, st)
        gpu.d2h(out, obuf.ptr, st)
        gpu.synchronize(st)
        want = oracle(data, None, Ellipsis if index is None else index, None, "var", 0)
        assert int(out["count"][0]) == data[Ellipsis if index is None else index].size
        check(moments.finalize(out.reshape(1, 1, 1)), want, f"G6 {dt} offset {off} {iname}")
