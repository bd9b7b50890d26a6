"""``Active.histogram`` on the device against ``np.histogram`` of the float64
copy of the masked selection (the selection is taken with NumPy and masked
with ``oracle.storage_ref.mask_missing``), per output; below, above and nan
come from direct comparisons, and ``histogram.bin_counts`` must agree.

Every comparison is exact: ``np.array_equal`` on int64, dtype and shape
included.  There are no tolerances.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import histogram as H
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu


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


def oracle(data, attrs, index, axis, edges, missing=None):
    """The components of the query: per output, np.histogram over the explicit
    float64 edges of the unmasked selection's float64 copy."""
    sel = np.ma.asarray(ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {})))
    nd = sel.ndim
    axes = tuple(range(nd)) if axis is None else tuple(a % nd for a in axis)
    kept = [d for d in range(nd) if d not in axes]
    final_shape = tuple(1 if d in axes else sel.shape[d] for d in range(nd))
    rows = np.ma.transpose(sel, kept + list(axes)).reshape(int(np.prod([sel.shape[d] for d in kept], dtype=np.int64)), -1)
    n = edges.size - 1
    out = {k: np.zeros(rows.shape[0], np.int64) for k in ("n", "below", "above", "nan")}
    counts = np.zeros((rows.shape[0], n), np.int64)
    for r in range(rows.shape[0]):
        x = rows[r].compressed().astype(np.float64)
        counts[r] = np.histogram(x, bins=edges)[0]
        out["n"][r] = x.size
        out["below"][r] = (x < edges[0]).sum()
        out["above"][r] = (x > edges[-1]).sum()
        out["nan"][r] = np.isnan(x).sum()
        second = H.bin_counts(x, edges)
        assert np.array_equal(second[0], counts[r])
        assert second[1:] == (out["below"][r], out["above"][r], out["nan"][r])
        assert counts[r].sum() + out["below"][r] + out["above"][r] + out["nan"][r] == x.size
    want = {k: v.reshape(final_shape) for k, v in out.items()}
    want["counts"] = counts.reshape(final_shape + (n,))
    want["bin_edges"] = edges
    return want


def same(got, want, what=""):
    assert isinstance(got, np.ndarray) and not isinstance(got, np.ma.MaskedArray), (what, type(got))
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), what


def check(got, want, components, what=""):
    if not components:
        return same(got, want["counts"], what)
    assert isinstance(got, dict) and set(got) == {"counts", "bin_edges", "n", "below", "above", "nan"}, what
    for k in want:
        same(got[k], want[k], (what, k))


def query(var, bins, rng, axis, index, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    a.histogram(bins=bins, range=rng, axis=axis)
    return a[index]


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
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
AXES = [None, (0,), (1,), (2,), (0, 2)]
# (bins, range) per dtype class: one bin; 7 bins whose edges float32 cannot hold; 64 bins of width
# 1.0; five explicit uneven edges.  Every range lies inside the data's spread.
SPECS = {
    "f": [(1, (280.0, 295.0)), (7, (270.1, 305.3)), (64, (256.0, 320.0)), ([265.5, 280.25, 288.0, 291.125, 310.0], None)],
    "i2": [(1, (-1000, 1500)), (7, (-2000.5, 2100.3)), (64, (-32, 32)), ([-2500.5, -100, 0, 7, 2000], None)],
    "u1": [(1, (50, 200)), (7, (20.1, 220.3)), (64, (100, 164)), ([15.5, 60, 128, 129, 230], None)],
    # 2^53 + 1 is no float64 (the edge is 2^53); values beyond 2^53 round to nearest on conversion
    "i8": [(1, (-2.0 ** 54, 2.0 ** 55)), (7, (-3.0e16, 2.5e16)), (64, (0, 64)),
           ([-3.3e16, -1.0e15, 0.5, 9007199254740993.0, 5.0e16], None)],
}


def spec_class(dt):
    dt = np.dtype(dt)
    return "f" if dt.kind == "f" else {2: "i2", 1: "u1", 8: "i8"}[dt.itemsize]


def spec_edges(spec):
    bins, rng = spec
    return H.edges(bins, rng)


def plant_values(dt, edges):
    """Each edge rounded to the dtype, and its two neighbours in the dtype."""
    dt = np.dtype(dt)
    nat = dt.newbyteorder("=")
    if dt.kind == "f":
        v = edges.astype(nat)
        return np.concatenate([v, np.nextafter(v, nat.type(-np.inf)), np.nextafter(v, nat.type(np.inf))])
    info = np.iinfo(nat)
    v = np.clip(np.rint(edges), float(info.min + 1), float(info.max - 1))
    v = np.array([int(t) for t in v], dtype=object)
    out = np.concatenate([v, v - 1, v + 1])
    return np.array([min(max(int(t), info.min), info.max) for t in out], dtype=nat)


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked):
    dt = np.dtype(dt)
    rng = np.random.default_rng(100 + DTYPES.index(dt.str if dt.str in DTYPES else "|u1"))
    if dt.kind == "f":
        # (a spread of 20: every selection of the sweep has values on both sides of every range)
        data = rng.normal(288.0, 20.0, SHAPE).astype(dt)
        fill, lo, hi = -999.0, 200.0, 380.0
    elif dt == np.dtype("<i8"):
        data = (rng.integers(-2 ** 55, 2 ** 55, SHAPE) * 2 + 1).astype(dt)
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 60), 2 ** 60
    elif dt == np.dtype("|u1"):
        data = rng.integers(10, 240, SHAPE).astype(dt)
        fill, lo, hi = 255, 5, 250
    else:
        data = rng.integers(-3000, 3000, SHAPE).astype(dt)
        fill, lo, hi = -32768, -3100, 3100
    attrs = {}
    flat = data.reshape(-1)
    if masked:
        flat[rng.choice(flat.size, flat.size // 50, replace=False)] = fill   # 2 %
        outl = rng.choice(flat.size, 40, replace=False)
        if dt.kind == "f" or dt == np.dtype("<i2"):   # a few beyond valid_min / valid_max
            flat[outl[:20]] = dt.type(lo - 50)
            flat[outl[20:]] = dt.type(hi + 50)
        one = lambda v: np.array([v], dtype=dt.newbyteorder("="))
        attrs = {"_FillValue": one(fill), "valid_min": one(lo), "valid_max": one(hi)}
    # every spec's edges, rounded to the dtype, with both neighbours
    plant = np.concatenate([plant_values(dt, spec_edges(s)) for s in SPECS[spec_class(dt)]])
    flat[rng.choice(flat.size, plant.size, replace=False)] = plant
    data.setflags(write=False)
    return data, attrs, make_var(data, CHUNKS, attrs, pad=fill)


@functools.lru_cache(maxsize=None)
def sweep_oracle(dt, masked, iname, axis, k):
    data, attrs, _ = sweep_var(dt, masked)
    index = dict(INDEXES)[iname]
    return oracle(data, attrs, NUMPY_INDEX.get(iname, index), axis, spec_edges(SPECS[spec_class(dt)][k]))


def _sweep_cases():
    k = 0
    for dt, (iname, index), axis, masked in itertools.product(DTYPES, INDEXES, AXES, (False, True)):
        spec = k % 4            # every dtype / index / axes / mask once; the four bin specs rotate
        comp = (k // 4) % 2 == 0
        k += 1
        yield pytest.param(dt, iname, index, axis, masked, spec, comp,
                           id=f"{dt[1:]}-{iname}-{'all' if axis is None else ''.join(map(str, axis))}-"
                              f"{'masked' if masked else 'plain'}-spec{spec}{'-comp' if comp else ''}")


@pytest.mark.parametrize("dt,iname,index,axis,masked,spec,comp", list(_sweep_cases()))
def test_sweep(gpu, dt, iname, index, axis, masked, spec, comp):
    data, attrs, var = sweep_var(dt, masked)
    bins, rng = SPECS[spec_class(dt)][spec]
    want = sweep_oracle(dt, masked, iname, axis, spec)
    assert want["below"].sum() > 0 and want["above"].sum() > 0     # the range sits inside the spread
    check(query(var, bins, rng, axis, index, comp), want, comp)


def test_sweep_plants_reach_the_edges():
    """The planted values put counts on both sides of every edge."""
    for dt in DTYPES:
        data, _, _ = sweep_var(dt, False)
        x = data.astype(np.float64)
        for s in SPECS[spec_class(dt)]:
            e = spec_edges(s)
            rounded = plant_values(dt, e)[:e.size].astype(np.float64)
            assert np.isin(rounded, x).all(), (dt, s)


# -- 2. shuffled storage ---------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (2,)], ids=["all", "2"])
@pytest.mark.parametrize("dt", ["<f4", "<f8"])
def test_shuffled_storage(gpu, dt, axis):
    rng = np.random.default_rng(7)
    data = rng.normal(288.0, 10.0, (64, 64, 16)).astype(dt)
    e = H.edges(16, (270.0, 300.0))
    data.reshape(-1)[:e.size] = e.astype(dt)
    var = make_var(data, (32, 64, 16), shuffle=True)
    for index in ((Ellipsis,), (slice(1, None), slice(None), slice(None))):
        check(query(var, 16, (270.0, 300.0), axis, index, True), oracle(data, None, index, axis, e), True)


# -- 3. NaN and infinities ---------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "fill"])
@pytest.mark.parametrize("dt", ["<f4", "<f8"])
def test_nan_and_infinities(gpu, dt, masked):
    rng = np.random.default_rng(3)
    data = rng.normal(0.0, 2.0, (20, 30, 17)).astype(dt)
    flat = data.reshape(-1)
    pos = rng.choice(flat.size, 400, replace=False)
    flat[pos[:50]] = np.nan
    flat[pos[50:90]] = np.inf
    flat[pos[90:120]] = -np.inf
    flat[pos[120:200]] = 3.0            # == hi: the last bin
    flat[pos[200:230]] = -3.0           # == lo: the first bin
    attrs = {}
    if masked:
        flat[pos[230:400]] = -999.0
        attrs = {"_FillValue": np.array([-999.0], dtype=dt)}
    var = make_var(data, (8, 16, 17), attrs, pad=-999.0)
    e = H.edges(12, (-3.0, 3.0))
    for axis in (None, (1,), (0, 2)):
        want = oracle(data, attrs, (Ellipsis,), axis, e)
        got = query(var, 12, (-3.0, 3.0), axis, Ellipsis, True)
        check(got, want, True, axis)
        assert got["nan"].sum() == 50 and got["above"].sum() >= 40 and got["below"].sum() >= 30
        assert got["counts"][..., -1].sum() >= 80
    # explicit edges (binary search) see the same values
    ee = np.array([-3.0, -1.0, -0.25, 0.0, 2.0, 3.0])
    check(query(var, ee, None, None, Ellipsis, True), oracle(data, attrs, (Ellipsis,), None, ee), True)


# -- 4. the LDS form's boundary: global edges and the generic form ----------------------
@pytest.mark.parametrize("axis", [None, (2,)], ids=["all", "2"])
@pytest.mark.parametrize("n_bins", [2048, 2049, 5000, "explicit3000"])
def test_lds_form_boundary(gpu, n_bins, axis):
    data, attrs, var = sweep_var("<f4", True)
    if n_bins == "explicit3000":
        rng = np.random.default_rng(9)
        bins, r = np.unique(rng.uniform(250.0, 330.0, 3001)), None
        assert bins.size == 3001
    else:
        bins, r = n_bins, (256.0, 320.0)
    e = H.edges(bins, r)
    check(query(var, bins, r, axis, Ellipsis, True), oracle(data, attrs, (Ellipsis,), axis, e), True)
    inner = INDEXES[1][1]
    check(query(var, bins, r, axis, inner), oracle(data, attrs, inner, axis, e), False)


# -- 5. one bin takes everything -------------------------------------------------------
@pytest.mark.parametrize("chunks", [(64, 64, 64), (32, 32, 32)], ids=["one-chunk", "eight-chunks"])
def test_one_bin_takes_everything(gpu, chunks):
    """262,144 equal values: the same-address worst case, and more than a
    16-bit count holds."""
    data = np.full((64, 64, 64), 5, "|u1")
    var = make_var(data, chunks)
    got = query(var, 4, (0, 8), None, Ellipsis, True)
    want = np.zeros((1, 1, 1, 4), np.int64)
    want[..., 2] = data.size
    same(got["counts"], want)
    assert got["n"].item() == data.size and got["below"].item() == got["above"].item() == got["nan"].item() == 0
    same(query(var, 1, (5, 5), None, Ellipsis), np.full((1, 1, 1, 1), data.size, np.int64))
    below = query(var, 4, (6, 8), None, Ellipsis, True)
    assert below["below"].item() == data.size and below["counts"].sum() == 0


# -- 6. several tiles per chunk, several chunks per workgroup -----------------------------
@functools.lru_cache(maxsize=None)
def tiles_var():
    rng = np.random.default_rng(13)
    data = rng.normal(288.0, 10.0, (64, 64, 128)).astype("<f4")
    return data, make_var(data, (32, 32, 64))


@pytest.mark.parametrize("index", [(Ellipsis,), (slice(1, -1), slice(1, -1), slice(1, -1))], ids=["whole", "inner"])
@pytest.mark.parametrize("wgs", [None, "3", "1"], ids=["grid-default", "grid-3", "grid-1"])
def test_tiles_and_chunks_per_workgroup(gpu, monkeypatch, wgs, index):
    """16 tiles per chunk (16 KiB tiles); with PYAS_HIST_WGS a workgroup walks
    tiles of several chunks and keeps its LDS table across them."""
    data, var = tiles_var()
    e = H.edges(64, (256.0, 320.0))
    want = oracle(data, None, index, None, e)
    if wgs is not None:
        monkeypatch.setenv("PYAS_HIST_WGS", wgs)
    base = query(var, 64, (256.0, 320.0), None, index, True)
    gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 16384)
    try:
        got = query(var, 64, (256.0, 320.0), None, index, True)
    finally:
        gpu.lib.pyas_ctx_set_tile_bytes(gpu.handle, 0)
    check(base, want, True)
    check(got, want, True)


def test_rows_change_inside_a_workgroup(gpu, monkeypatch):
    """pyas_hist_axes with every dim reduced and out_offsets / out_index given:
    one workgroup walks chunks of alternating rows and adds its LDS table
    whenever the row changes."""
    from pyactivestorage_amd import engine
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    monkeypatch.setenv("PYAS_HIST_WGS", "1")
    rng = np.random.default_rng(17)
    chunks = rng.normal(0.0, 1.0, (6, 8, 8, 8)).astype("<f4")
    e = H.edges(8, (-2.0, 2.0))
    st = gpu.thread_stream()
    buf = DeviceBuffer(gpu, chunks.nbytes)
    gpu.h2d(buf.ptr, chunks, st)
    plan = ReductionPlan(gpu, chunks.dtype, (8, 8, 8), buf.ptr, np.arange(6, dtype=np.int64) * 2048, stream=st)
    out_off = np.arange(6, dtype=np.int64)
    out_index = np.array([2, 0, 2, 1, 1, 2], dtype=np.int64)
    meta = np.concatenate([out_off, out_index])
    mbuf, ebuf, tbuf = DeviceBuffer(gpu, meta.nbytes), DeviceBuffer(gpu, e.nbytes), DeviceBuffer(gpu, 3 * 11 * 8)
    gpu.h2d(mbuf.ptr, meta, st)
    gpu.h2d(ebuf.ptr, e, st)
    tab = np.full((3, 11), -1, np.int64)
    for index_ptr, rows in ((mbuf.ptr + 48, out_index), (None, None)):
        engine.hist_reset(gpu, tbuf.ptr, 3, 8, st)
        n_chunks = 6 if rows is not None else 3      # identity: rows 0, 1, 2
        if rows is None:
            plan = ReductionPlan(gpu, chunks.dtype, (8, 8, 8), buf.ptr, np.arange(3, dtype=np.int64) * 2048, stream=st)
            rows = np.arange(3)
        engine.hist_axes(gpu, plan.batch, plan.mask_up.struct, ebuf.ptr, 8, (e[0], 8 / (e[-1] - e[0])), 0b111,
                         mbuf.ptr, index_ptr, tbuf.ptr, st)
        gpu.d2h(tab, tbuf.ptr, st)
        gpu.synchronize(st)
        want = np.zeros((3, 11), np.int64)
        for c in range(n_chunks):
            cnt, below, above, nan = H.bin_counts(chunks[c], e)
            want[rows[c], :8] += cnt
            want[rows[c], 8:] += (below, above, nan)
        same(tab, want)


# -- 7. rank 1 and rank 4 -----------------------------------------------------------------
def test_rank_1(gpu):
    rng = np.random.default_rng(19)
    data = rng.normal(0.0, 1.0, 1000).astype("<f8")
    var = make_var(data, (96,))
    e = H.edges(20, (-2.0, 2.5))
    for index in ((Ellipsis,), (slice(5, 990, 3),), ([3, 4, 500, 999],)):
        check(query(var, 20, (-2.0, 2.5), None, index, True), oracle(data, None, index, None, e), True)
    # a partial-axis query of a rank-1 variable reduces nothing: one element per output
    check(query(var, 20, (-2.0, 2.5), (), (slice(90, 110),), True), oracle(data, None, (slice(90, 110),), (), e), True)


def test_rank_4(gpu):
    rng = np.random.default_rng(23)
    data = rng.integers(-50, 50, (5, 6, 7, 9)).astype("<i4")
    attrs = {"_FillValue": np.array([-7], "<i4")}
    var = make_var(data, (3, 4, 4, 5), attrs, pad=-7)
    e = H.edges(10, (-40, 41))
    for axis in (None, (1, 3), (0,), (3,), (0, 1, 2)):
        for index in ((Ellipsis,), (slice(1, None), slice(None), [0, 2, 6], slice(2, 8))):
            check(query(var, 10, (-40, 41), axis, index, True), oracle(data, attrs, index, axis, e), True,
                  (axis, index))


# -- 8. range=None ---------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["plain", "resident"])
def test_range_none(gpu, resident):
    from pyactivestorage_amd.active import release_resident
    data, attrs, _ = sweep_var("<f4", True)
    var = make_var(data, CHUNKS, attrs, pad=-999.0)
    try:
        for index in ((Ellipsis,), INDEXES[1][1]):
            x = np.ma.asarray(ref.mask_missing(data[index], get_missing_attributes(attrs))).compressed().astype(np.float64)
            wc, we = np.histogram(x, bins=9)
            got = query(var, 9, None, None, index, True, resident=resident)
            same(got["bin_edges"], we)
            same(got["counts"], wc.astype(np.int64).reshape(1, 1, 1, 9))
            assert got["below"].item() == got["above"].item() == 0 and got["n"].item() == x.size
            # per-axis counts share the whole selection's range
            part = query(var, 9, None, (0,), index, True, resident=resident)
            check(part, oracle(data, attrs, index, (0,), we), True)
    finally:
        release_resident(var)


def test_range_none_constant_all_masked_and_nan(gpu):
    const = np.full((20, 30, 17), 287.65, "<f4")
    got = query(make_var(const, (8, 12, 20), pad=1.0), 6, None, None, Ellipsis, True)
    wc, we = np.histogram(const.astype(np.float64), bins=6)
    same(got["bin_edges"], we)
    same(got["counts"], wc.astype(np.int64).reshape(1, 1, 1, 6))
    attrs = {"_FillValue": np.array([287.65], "<f4")}
    got = query(make_var(const, (8, 12, 20), attrs, pad=1.0), 6, None, (1,), Ellipsis, True)
    same(got["bin_edges"], np.linspace(0.0, 1.0, 7))
    same(got["counts"], np.zeros((20, 1, 17, 6), np.int64))
    same(got["n"], np.zeros((20, 1, 17), np.int64))
    same(query(make_var(const, (8, 12, 20), attrs, pad=1.0), 6, None, None, Ellipsis), np.zeros((1, 1, 1, 6), np.int64))
    bad = const.copy()
    bad[3, 4, 5] = np.nan
    with pytest.raises(ValueError):
        query(make_var(bad, (8, 12, 20)), 6, None, None, Ellipsis)
    bad[3, 4, 5] = np.inf
    with pytest.raises(ValueError):
        query(make_var(bad, (8, 12, 20)), 6, None, None, Ellipsis)


# -- 9. the same bytes, and settings that do not leak ------------------------------------------
def test_same_bytes_and_no_leak(gpu):
    from pyactivestorage_amd.active import release_resident
    data, attrs, _ = sweep_var("<f8", True)
    var = make_var(data, CHUNKS, attrs, pad=-999.0)
    bins, rng = SPECS["f"][1]
    try:
        for axis in (None, (1,)):
            runs = [query(var, bins, rng, axis, Ellipsis) for _ in range(2)]
            a = Active(var, resident=True)
            for _ in range(3):
                a.histogram(bins, rng, axis=axis)
                runs.append(a[...])
            for r in runs[1:]:
                assert r.tobytes() == runs[0].tobytes()
            same(runs[0], oracle(data, attrs, (Ellipsis,), axis, H.edges(bins, rng))["counts"])
            # the settings hold for one query
            assert a._hist is None and a._method is None
            plain = Active(var, resident=True).mean(axis=axis)[...]
            after = a.mean(axis=axis)[...]
            assert type(after) is type(plain) and after.dtype == plain.dtype
            assert np.ma.getdata(after).tobytes() == np.ma.getdata(plain).tobytes()
            assert np.array_equal(np.ma.getmaskarray(after), np.ma.getmaskarray(plain))
            a.components = True
            a.histogram(bins, rng, axis=axis)
            comp = a[...]
            a.components = False
            same(comp["counts"], runs[0])
    finally:
        release_resident(var)


# -- 10. errors ----------------------------------------------------------------------------------
def test_errors(gpu, monkeypatch):
    data, attrs, var = sweep_var("<f4", True)
    for kw in (dict(bins=0), dict(bins=-1), dict(bins=1.5), dict(bins=True), dict(bins=[1.0]), dict(bins=[0, 1, 1]),
               dict(bins=[0, np.inf]), dict(bins=[2, 1]), dict(bins=4, range=(0, np.inf)), dict(bins=4, range=(np.nan, 1)),
               dict(bins=4, range=(3, 2)), dict(bins=(1 << 20) + 1, range=(0, 1)), dict(bins=(1 << 20) + 1)):
        with pytest.raises(ValueError):
            Active(var).histogram(**kw)[...]
    a = Active(var)
    a.weights = {0: np.ones(SHAPE[0])}
    a.histogram(4, (250, 300))
    with pytest.raises(ValueError):
        a[...]
    with pytest.raises(ValueError):
        Active(var).mean(weights={0: np.ones(SHAPE[0])}).histogram(4, (250, 300))[...]
    with pytest.raises(NotImplementedError):
        Active(var, group=object()).histogram(4, (250, 300))[...]
    with pytest.raises(IndexError):
        Active(var).histogram(4, (250, 300))[3, :, :]
    with pytest.raises(IndexError):
        Active(var).histogram(4, None, axis=(1,))[:, :, 0]
    # the table cap: n_outputs x (n_bins + 3) x 8 bytes; the message names both sizes
    monkeypatch.setattr(H, "TABLE_CAP_BYTES", 15 * 37 * 7 * 8 - 1)
    with pytest.raises(ValueError, match=rf"{15 * 37 * 7 * 8}.*{15 * 37 * 7 * 8 - 1}"):
        Active(var).histogram(4, (250, 300), axis=(1,))[...]
    with pytest.raises(ValueError):
        Active(var).histogram(4, None, axis=(1,))[...]          # before the range is looked for
    monkeypatch.setattr(H, "TABLE_CAP_BYTES", 15 * 37 * 7 * 8)
    got = Active(var).histogram(4, (250, 300), axis=(1,))[...]
    same(got, oracle(data, attrs, (Ellipsis,), (1,), H.edges(4, (250, 300)))["counts"])
    assert H.TABLE_CAP_BYTES == 15 * 37 * 7 * 8


# -- 11. branches the shapes above do not reach (the cases of tests/_stats_gaps.py) -----------
from tests import _stats_gaps as G   # noqa: E402

MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


def gap_range(dt):
    if dt in G.G5_HIST_RANGE:
        return G.G5_HIST_RANGE[dt]
    return G.HIST_RANGE if np.dtype(dt).kind == "f" else (-1500, 1500)     # <i2 over -3000..3000


@functools.lru_cache(maxsize=None)
def gap_var(group, name, dt="<f4", masked=False, shuffle=None):
    """The case's data with every edge of its 4 bins planted (rounded to the
    dtype, with both neighbours); the data's spread lies on both sides of the range."""
    data, attrs = G.single(group, name, dt, masked)
    _, chunks, _, _, shuffled = G.case(group, name)
    shuffle = shuffled if shuffle is None else shuffle
    rng = gap_range(dt)
    e = H.edges(G.HIST_BINS, rng)
    data = G.planted(data, attrs, plant_values(dt, e))
    return data, attrs, make_var(data, chunks, attrs, shuffle=shuffle, pad=G.fill_of(attrs, dt)), rng, e


def gap_check(group, name, dt, masked, iname, axis, shuffle=None):
    data, attrs, var, rng, e = gap_var(group, name, dt, masked, shuffle)
    index = G.index_of(group, name, iname)
    want = oracle(data, attrs, index, axis, e)
    check(query(var, G.HIST_BINS, rng, axis, index, True), want, True, f"{group} {name} {dt} {iname} {G.axis_id(axis)}")
    return want


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(gpu, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in its launch."""
    data, attrs, var, rng, e = gap_var("G2", name, "<f4", masked)
    k = G.G2_SECOND_TRIP
    want = oracle(data, attrs, (Ellipsis,), (0,), e)
    assert want["below"].sum() > 0 and want["above"].sum() > 0
    got = query(var, G.HIST_BINS, rng, (0,), Ellipsis, True)
    for key in ("n", "below", "above", "nan"):
        same(got[key].reshape(-1)[k:], want[key].reshape(-1)[k:], f"G2 {name} {key}: the second trip, outputs {k}..16899")
    same(got["counts"].reshape(-1, G.HIST_BINS)[k:], want["counts"].reshape(-1, G.HIST_BINS)[k:],
         f"G2 {name} counts: the second trip, outputs {k}..16899")
    check(got, want, True, f"G2 {name}: every output")


@MASKED
@pytest.mark.parametrize("iname", ["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=G.axis_id)
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_shuffled_chunks_of_odd_size(gpu, dt, axis, iname, masked):
    """Shuffled chunks of 105 elements: hist_run_shuffled's per-element fallback."""
    want = gap_check("G3", "odd", dt, masked, iname, axis)
    assert want["below"].sum() > 0 and want["above"].sum() > 0


@pytest.mark.parametrize("iname", list(G.G3_RUNS))
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_runs_inside_a_shuffled_chunk(gpu, dt, iname):
    gap_check("G3", "runs", dt, False, iname, None)


@MASKED
def test_g4_rank_8(gpu, masked):
    for iname, _, axis, _ in G.combos("G4", "8d"):
        want = gap_check("G4", "8d", "<f4", masked, iname, axis)
        assert want["below"].sum() > 0 and want["above"].sum() > 0


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    for axis in (None, (1,)):
        want = gap_check("G5", "dtypes", dt, masked, "whole", axis, shuffle)
        assert want["below"].sum() > 0 and want["above"].sum() > 0
        assert (want["counts"].reshape(-1, G.HIST_BINS).sum(axis=0) > 0).all()


@pytest.mark.parametrize("dt,off", G.G6_CASES)
def test_g6_base_misaligned(gpu, dt, off):
    """One chunk ``off`` bytes into its buffer, every dim reduced, through
    pyas_hist_axes itself: the head and tail of hist_run_plain."""
    from pyactivestorage_amd import engine
    from pyactivestorage_amd.device import DeviceBuffer
    rng = G.HIST_RANGE if dt == "<f4" else (64, 192)
    e = H.edges(G.HIST_BINS, rng)
    data = G.planted(G.g6_chunk(dt), None, plant_values(dt, e))
    for iname, index in G.G6_INDEXES.items():
        st, buf, plan = G.misaligned_plan(gpu, data, off, index)
        ebuf, tbuf = DeviceBuffer(gpu, e.nbytes), DeviceBuffer(gpu, (G.HIST_BINS + 3) * 8)
        gpu.h2d(ebuf.ptr, e, st)
        engine.hist_reset(gpu, tbuf.ptr, 1, G.HIST_BINS, st)
        engine.hist_axes(gpu, plan.batch, plan.mask_up.struct, ebuf.ptr, G.HIST_BINS,
                         (e[0], G.HIST_BINS / (e[-1] - e[0])), 0b111, None, None, tbuf.ptr, st)
        tab = np.full((1, G.HIST_BINS + 3), -1, np.int64)
        gpu.d2h(tab, tbuf.ptr, st)
        gpu.synchronize(st)
        cnt, below, above, nan = H.bin_counts(data[Ellipsis if index is None else index].astype(np.float64), e)
        want = np.concatenate([cnt, [below, above, nan]]).astype(np.int64).reshape(1, -1)
        assert below > 0 and above > 0 and (cnt > 0).all()
        same(tab, want, f"G6 {dt} offset {off} {iname}")
