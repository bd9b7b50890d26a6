"""float64 sums and means of the core reductions against the exactly rounded
reference (``math.fsum`` of the masked selection), held to the derived
``tests/_compare.sum_bound``: (n + 2) u sum|x| with u = 2**-53, and for a
mean that over n plus two roundings of |mean|.  Every path below carries f64
end to end (``GroupSum<double>`` is double, the partial's sum field is f64,
the combines are templated on T), so any float32 temporary (a tree helper, a
compact record written through the wrong type, a rounding to the wrong
dtype, a division in f32, a host-side astype, a CBOR float32) costs about
3e-8 relative and falls outside the bound by seven orders of magnitude.

The worst-case bound grows as n * sum|x|, so the shapes are small: at most
1024 values per output wherever an element-level fault must show; the
300-chunk totals (38400 values) only look for combine-level faults.  The
data are uniform draws with full 52-bit mantissas (plus planted fill values).
The last test prints, per path, the worst observed error/bound.
"""
import concurrent.futures
import ctypes

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import _lib, engine, selection
from pyactivestorage_amd import active as active_mod
from pyactivestorage_amd import storage as pas
from pyactivestorage_amd.active import Active, release_resident
from tests._compare import (U64, assert_reduction_close, assert_within, exact_reference, shuffle_bytes,
                            sum_bound)
from tests.test_gpu_axes_stream import _chunks, _partials
from tests.test_gpu_moments import make_var

pytestmark = pytest.mark.gpu

FILL, VMIN, VMAX = -999.0, -40.0, 140.0
MISS = (FILL, None, VMIN, VMAX)
ATTRS = {"_FillValue": np.array([FILL]), "valid_min": np.array([VMIN]), "valid_max": np.array([VMAX])}
RATIOS = {}


def _note(path, r):
    RATIOS[path] = max(RATIOS.get(path, 0.0), r)


def _data(rng, shape, dt="<f8", masked=False, cancel=False):
    """uniform(-50, 150) in f64; ``cancel``: the second half along dim 0
    mirrors the first to within 1e-9 relative, so every sum over dim 0
    cancels to about 1e-9 of sum|x|; ``masked``: 5 % fill values (others
    fall outside the valid range by themselves)."""
    a = rng.uniform(-50, 150, size=shape)
    if cancel:
        h = shape[0] // 2
        a[h:2 * h] = -a[:h] * (1 + 1e-9 * rng.uniform(-1, 1, size=a[:h].shape))
    if masked:
        a.reshape(-1)[rng.random(a.size) < 0.05] = FILL
    return a.astype(dt)


def _masked(a, miss):
    return ref.mask_missing(a.astype(a.dtype.newbyteorder("=")), miss if miss else (None,) * 4)


# ---------------------------------------------------------------------------
# the drop-in reduce_chunk_bytes
# ---------------------------------------------------------------------------
SELS = {
    (6, 5, 7): [("whole", np.s_[0:6, 0:5, 0:7]), ("box", np.s_[1:4, 0:5, 0:7]), ("inner", np.s_[2:5, 1:5, 2:6]),
                ("strided", np.s_[0:6:2, 1:5:3, 0:7:4]), ("listed", (slice(None), [0, 1, 4], slice(None)))],
    (8, 12, 32): [("whole", np.s_[0:8, 0:12, 0:32]), ("box", np.s_[2:7, 0:12, 0:32]),
                  ("inner", np.s_[1:8, 3:11, 4:29]), ("strided", np.s_[1:8:3, 0:12:2, 3:32:5]),
                  ("listed", (slice(None), [0, 3, 4, 11], slice(None)))],
}
METHODS = [np.ma.sum, np.ma.mean, np.sum, np.mean]


@pytest.mark.parametrize("cancel", [False, True])
@pytest.mark.parametrize("dt", ["<f8", ">f8"])
@pytest.mark.parametrize("shape", list(SELS))
def test_dropin_reduce_chunk_bytes(gpu, shape, dt, cancel):
    """k_reduce (whole chunk), run_spans / run_rows_any (contiguous boxes)
    and the generic walk (strided, listed), plain and byte-shuffled, with and
    without masks, over axis None, (1,) and (0, 2)."""
    rng = np.random.default_rng(len(shape) + shape[2] + (dt == ">f8") + 2 * cancel)
    for masked in (False, True):
        arr = _data(rng, shape, dt, masked, cancel)
        miss = MISS if masked else (None,) * 4
        for shuf in (False, True):
            raw = shuffle_bytes(arr, 8) if shuf else arr.tobytes()
            gf = [pas.Shuffle(8)] if shuf else None
            for name, sel in SELS[shape]:
                vals = _masked(arr, miss)[sel]
                for axis in (None, (1,), (0, 2)):
                    ex_n = exact_reference(vals, axis)["n"]
                    for method in METHODS:
                        kind = "mean" if method.__name__ == "mean" else "sum"
                        got, gn = pas.reduce_chunk_bytes(raw, None, gf, miss, dt, shape, "C", sel, axis, method)
                        what = f"{dt} {shape} {name} shuf={shuf} masked={masked} axis={axis} {method.__name__}"
                        assert np.asarray(got).dtype == np.float64, what
                        np.testing.assert_array_equal(np.asarray(gn).reshape(-1), ex_n, err_msg=what)
                        ok = ~np.ma.getmaskarray(got).reshape(-1)
                        np.testing.assert_array_equal(ok, ex_n > 0, err_msg=what)
                        r = assert_reduction_close(got, vals, axis, dt, kind, what, ok=ok)
                        _note(f"drop-in {name}{' cancelling' if cancel else ''} {kind}", r)


# ---------------------------------------------------------------------------
# per-chunk partials through engine.reduce_axes: every partial-axis kernel
# the host can select for f8, 32-byte partials and 16-byte Rec<double> records
# ---------------------------------------------------------------------------
def _axes_run(ctx, dt, shape, chunks, axes, miss, shuf, sels, rec):
    """One pyas_reduce_axes(_ex) call over ``chunks`` (whole, or the boxes /
    strided selections ``sels``); ``rec`` 0: 32-byte partials, REC_SUM: the
    compact records, returned as (sum, count) arrays per chunk."""
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    st = ctx.thread_stream()
    es, n, cbytes = dt.itemsize, len(chunks), chunks[0].nbytes
    offsets = np.arange(n, dtype=np.int64) * (cbytes + 16)
    blob = np.zeros(int(offsets[-1]) + cbytes + 16, dtype=np.uint8)
    for k, a in enumerate(chunks):
        raw = shuffle_bytes(a, es) if shuf else a.tobytes()
        blob[offsets[k]:offsets[k] + cbytes] = np.frombuffer(raw, np.uint8)
    dbuf = DeviceBuffer(ctx, blob.nbytes)
    ctx.h2d(dbuf.ptr, blob, st)
    csels = [selection.normalize(s, shape) for s in sels] if sels else None
    plan = ReductionPlan(ctx, dt, shape, dbuf.ptr, offsets, selections=csels, missing=miss, stream=st,
                         shuffle=es if shuf else 0)
    cshape = [c.shape for c in csels] if csels else [shape] * n
    n_outs = [int(np.prod([1 if d in axes else cs[d] for d in range(len(shape))])) for cs in cshape]
    out_offs = np.concatenate([[0], np.cumsum(n_outs)[:-1]]).astype(np.int64)
    total = int(sum(n_outs))
    offs = DeviceBuffer(ctx, out_offs.nbytes)
    ctx.h2d(offs.ptr, out_offs, st)
    rb = _lib.rec_nbytes(es, rec) if rec else _lib.PARTIAL_NBYTES
    out = DeviceBuffer(ctx, total * rb)
    engine.reduce_axes(ctx, plan.batch, plan.mask_up.struct, sum(1 << a for a in axes), offs.ptr, out.ptr, st,
                       rec=rec)
    host = np.zeros(total * rb, dtype=np.uint8)
    ctx.d2h(host, out.ptr, st)
    ctx.synchronize(st)
    for b in (dbuf, offs, out):
        b.free()
    if rec:
        assert rb == 16
        rows = host.reshape(total, 16)
        sums = rows[:, :8].copy().view("<f8").reshape(-1)
        counts = rows[:, 8:12].copy().view("<i4").reshape(-1)
    else:
        p = host.view(engine.partial_dtype(dt))
        sums, counts = p["sum"], p["count"]
    return [(sums[o:o + m], counts[o:o + m]) for o, m in zip(out_offs, n_outs)]


def _box(shape):           # a cut covering more than half the chunk
    return tuple(slice(1, n) if d != 1 else slice(0, n - 1) for d, n in enumerate(shape))


def _strided(shape):       # strided kept and reduced dims: the generic k_reduce_axes walk
    return tuple(slice(0, n, 2) for n in shape)


def _slab_accepts(shape, axes, es):
    """The host's own test for k_axes_shuf_slab (pyas_reduce_axes_ex): the
    reduced dim between one kept-outer and a kept-inner run of 64 or 128
    columns, RB = min(16 KiB / (KI * es), RI) rows rounded down to 4 per
    tile, RI a multiple of RB, whole 1 KiB plane loads, and at least 256
    column items (split 1).  The library reports no kernel choice, so the
    test restates the rule for the shape it uses."""
    if len(shape) != 3 or axes != (1,):
        return False
    ko, ri, ki = shape
    rb = min(16384 // (ki * es), ri)
    rb -= rb % 4
    return (ki in (64, 128) and rb >= 4 and ri % rb == 0 and (rb * ki) % 1024 == 0
            and ko * ki // (16 // es) >= 256)


# (path, shape, axes, env, selection of every other chunk, shuffled, env of a
#  path that must give the same bytes: the kernels documented as bit-identical)
KERNELS = [
    ("dense column", (8, 32, 64), (0,), {"PYAS_COL_STREAM": "0"}, None, False, None),
    ("dense column shuffled", (8, 32, 64), (0,), {"PYAS_COL_STREAM": "0", "PYAS_SHUF_SLAB": "0"}, None, True, None),
    ("column stream", (8, 64, 64), (0,), {"PYAS_COL_STREAM": "3"}, None, False, {"PYAS_COL_STREAM": "0"}),
    ("shuffled slab", (16, 64, 64), (1,), {"PYAS_SHUF_SLAB": "1"}, None, True, {"PYAS_SHUF_SLAB": "0"}),
    ("LDS row", (8, 16, 32), (2,), {"PYAS_ROW_LDS": "2"}, None, False, None),
    ("butterfly row", (8, 16, 64), (2,), {"PYAS_ROW_LDS": "0"}, None, False, None),
    ("cut column", (8, 32, 64), (0,), {"PYAS_AXES_CUTS": "1"}, _box, False, None),
    ("cut LDS row", (8, 16, 32), (2,), {"PYAS_AXES_CUTS": "1", "PYAS_ROW_LDS": "2"}, _box, False, None),
    ("generic strided", (6, 10, 14), (0, 2), {}, _strided, False, None),
    ("generic odd extents", (6, 10, 14), (0, 2), {}, None, False, None),
]


@pytest.mark.parametrize("dt", ["<f8", ">f8"])
@pytest.mark.parametrize("kernel", range(len(KERNELS)), ids=[k[0].replace(" ", "-") for k in KERNELS])
def test_axes_partials_and_records(gpu, monkeypatch, kernel, dt):
    path, shape, axes, env, cut, shuf, sibling = KERNELS[kernel]
    dt = np.dtype(dt)
    assert _slab_accepts(shape, axes, dt.itemsize) == (path == "shuffled slab")
    rng = np.random.default_rng(40 + kernel)
    n = 7
    full = tuple(slice(0, m) for m in shape)
    sels = [full if k % 2 == 0 else cut(shape) for k in range(n)] if cut else None
    for masked, cancel in ((False, False), (True, False), (True, True)):
        chunks = [_data(rng, shape, dt, masked, cancel and 0 in axes) for _ in range(n)]
        miss = MISS if masked else None
        exs = [exact_reference(_masked(a, miss)[sels[k] if sels else full], axes) for k, a in enumerate(chunks)]
        for rec in (0, _lib.REC_SUM):
            for k, v in env.items():
                monkeypatch.setenv(k, v)
            got = _axes_run(gpu, dt, shape, chunks, axes, miss, shuf, sels, rec)
            if sibling:
                for k, v in sibling.items():
                    monkeypatch.setenv(k, v)
                other = _axes_run(gpu, dt, shape, chunks, axes, miss, shuf, sels, rec)
                for g, o in zip(got, other):
                    assert g[0].tobytes() == o[0].tobytes() and g[1].tobytes() == o[1].tobytes(), (path, rec)
            for k, ex in enumerate(exs):
                what = f"{path} {dt} masked={masked} cancel={cancel} rec={rec} chunk {k}"
                np.testing.assert_array_equal(got[k][1], ex["n"], err_msg=what)
                assert ex["n"].max() <= 1024
                r = assert_within(got[k][0], ex["exact"], sum_bound(dt, ex["n"], ex["abs_sum"]), what)
                _note(f"partials {path}" + (" records" if rec else ""), r)


@pytest.mark.parametrize("stream_env", [0, 3])
def test_column_partials_with_planted_values(gpu, monkeypatch, stream_env):
    """The column kernels on the stream module's own chunks (fill values,
    both zeros), through that module's launcher."""
    from pyactivestorage_amd.device import get_context
    ctx = get_context(0)
    st = ctx.thread_stream()
    dt = np.dtype("<f8")
    shape, axes = (8, 64, 64), (0,)
    chunks = _chunks(dt, shape, 5, np.random.default_rng(9), nan=False)
    miss = (-999, None, -50, 140)
    got = _partials(ctx, st, dt, shape, chunks, axes, miss, False, False, stream_env, monkeypatch)
    for k, a in enumerate(chunks):
        ex = exact_reference(_masked(a, miss), axes)
        np.testing.assert_array_equal(got[k]["count"], ex["n"])
        r = assert_within(got[k]["sum"], ex["exact"], sum_bound(dt, ex["n"], ex["abs_sum"]), f"chunk {k}")
        _note("partials column (stream module's chunks)", r)


# ---------------------------------------------------------------------------
# combines
# ---------------------------------------------------------------------------
BIG_SHAPE, BIG_CHUNKS = (20, 24, 80), (4, 4, 8)        # 5 * 6 * 10 = 300 chunks


@pytest.fixture(scope="module")
def big():
    rng = np.random.default_rng(300)
    data = _data(rng, BIG_SHAPE, "<f8", masked=True)
    return data, _masked(data, MISS)


@pytest.mark.parametrize("shuf", [False, True])
def test_whole_variable_total(gpu, big, shuf):
    """300 chunks: k_finish with two blocks, a group fold and the last-arrival
    total; through Active (sum and mean) and through ReductionPlan with
    round_to_var on and off.  38400 values: combine-level faults only."""
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    data, vals = big
    var = make_var(data, BIG_CHUNKS, ATTRS, shuffle=shuf)
    for method in ("sum", "mean"):
        a = Active(var)
        getattr(a, method)()
        got = a[...]
        assert got.dtype == np.float64 and got.shape == (1, 1, 1)
        _note(f"Active whole-variable {method}", assert_reduction_close(got, vals, None, "<f8", method,
                                                                         f"Active {method} shuf={shuf}"))
    st = gpu.thread_stream()
    blocks = [np.ascontiguousarray(data[tuple(slice(i * c, (i + 1) * c) for i, c in zip(cc, BIG_CHUNKS))])
              for cc in np.ndindex(5, 6, 10)]
    blob = np.concatenate([np.frombuffer(shuffle_bytes(b, 8) if shuf else b.tobytes(), np.uint8) for b in blocks])
    dbuf = DeviceBuffer(gpu, blob.nbytes)
    gpu.h2d(dbuf.ptr, blob, st)
    offsets = np.arange(300, dtype=np.int64) * blocks[0].nbytes
    ex = exact_reference(vals)
    for rtv in (True, False):
        plan = ReductionPlan(gpu, np.dtype("<f8"), BIG_CHUNKS, dbuf.ptr, offsets, missing=MISS, round_to_var=rtv,
                             stream=st, shuffle=8 if shuf else 0)
        plan.launch(st)
        tot = plan.read_total(st)[0]
        assert int(tot["count"]) == int(ex["n"][0])
        _note("ReductionPlan total", assert_within(np.array([tot["sum"]]), ex["exact"],
                                                   sum_bound("<f8", ex["n"], ex["abs_sum"]),
                                                   f"plan total round_to_var={rtv} shuf={shuf}"))
        parts = plan.read_chunk_partials(st)
        for k in (0, 151, 299):
            e = exact_reference(_masked(blocks[k], MISS))
            _note("ReductionPlan chunk partials", assert_within(
                np.array([parts[k]["sum"]]), e["exact"], sum_bound("<f8", e["n"], e["abs_sum"]), f"chunk {k}"))
    dbuf.free()


# shape, chunks, axis, index: the leading axis reduced over chunk layers
GRID_CASES = [
    ("few layers", (20, 24, 80), (4, 4, 8), (0,), np.s_[...]),
    ("box", (20, 24, 80), (4, 4, 8), (0,), np.s_[2:19, 3:22, 5:77]),
    ("wave: 130 layers", (130, 8, 16), (1, 4, 16), (0,), np.s_[...]),
    ("column fold", (32, 64, 64), (8, 16, 64), (0,), np.s_[...]),
    ("LDS row fold", (32, 32, 32), (8, 16, 32), (2,), np.s_[...]),
]


@pytest.mark.parametrize("fold", [True, False])
@pytest.mark.parametrize("case", range(len(GRID_CASES)), ids=[c[0].replace(" ", "-") for c in GRID_CASES])
def test_partial_axis_queries(gpu, monkeypatch, case, fold):
    """Active partial-axis sum and mean (formatted on the device by
    pyas_format_partials) with the fold kernels on (_AXES_FOLD) and on the
    two-step path (compact records, k_combine_grid and its wave form)."""
    name, shape, chunks, axis, index = GRID_CASES[case]
    monkeypatch.setattr(active_mod, "_AXES_FOLD", fold)
    folded, real = [], engine.reduce_axes_grid

    def spy(*a, **k):
        real(*a, **k)          # NotImplementedError: the geometry has no fold kernel
        folded.append(1)
    monkeypatch.setattr(engine, "reduce_axes_grid", spy)
    gpu.set_fold_min_blocks(1)
    try:
        rng = np.random.default_rng(70 + case)
        for dt, shuf, cancel in (("<f8", False, False), (">f8", True, False), ("<f8", False, True)):
            data = _data(rng, shape, dt, masked=True, cancel=cancel and 0 in axis)
            vals = _masked(data, MISS)[index]
            var = make_var(data, chunks, ATTRS, shuffle=shuf)
            for method in ("sum", "mean"):
                a = Active(var)
                getattr(a, method)(axis=axis)
                del folded[:]
                got = a[index]
                # whole-chunk grids must take the fold kernel when it is on; a box never does
                assert len(folded) == (1 if fold and index is Ellipsis else 0), (name, fold, folded)
                path = "folded in the kernel" if folded else "two-step"
                what = f"{name} {path} {dt} shuf={shuf} cancel={cancel} {method}"
                assert got.dtype == np.float64, what
                n = exact_reference(vals, axis)["n"]
                assert n.max() <= 1024
                ok = ~np.ma.getmaskarray(got).reshape(-1)
                np.testing.assert_array_equal(ok, n > 0, err_msg=what)
                _note(f"Active partial-axis {name}, {path}, {method}",
                      assert_reduction_close(got, vals, axis, dt, method, what, ok=ok))
    finally:
        gpu.set_fold_min_blocks(0)


@pytest.mark.parametrize("rec", [0, _lib.REC_SUM])
def test_combine_segments_and_device_format(gpu, rec):
    """pyas_combine_segments over a listed choice of chunks (each output
    combines that output of chunks 5, 0, 3, 6, in that order), from 32-byte
    partials and from 16-byte records, round_to_var on and off; then the mean
    formatted on the device (pyas_format_partials)."""
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    dt = np.dtype("<f8")
    shape, axes, listed = (6, 10, 14), (0, 2), [5, 0, 3, 6]
    rng = np.random.default_rng(55)
    chunks = [_data(rng, shape, dt, masked=True) for _ in range(7)]
    st = gpu.thread_stream()
    blob = np.concatenate([np.frombuffer(a.tobytes(), np.uint8) for a in chunks])
    dbuf = DeviceBuffer(gpu, blob.nbytes)
    gpu.h2d(dbuf.ptr, blob, st)
    plan = ReductionPlan(gpu, dt, shape, dbuf.ptr, np.arange(7, dtype=np.int64) * chunks[0].nbytes, missing=MISS,
                         stream=st)
    n_out = shape[1]
    index = np.array([c * n_out + j for j in range(n_out) for c in listed], dtype=np.int64)
    seg = np.arange(n_out + 1, dtype=np.int64) * len(listed)
    meta = np.concatenate([np.arange(7, dtype=np.int64) * n_out, index, seg])
    mbuf = DeviceBuffer(gpu, meta.nbytes)
    gpu.h2d(mbuf.ptr, meta, st)
    rb = _lib.rec_nbytes(8, rec) if rec else _lib.PARTIAL_NBYTES
    parts = DeviceBuffer(gpu, 7 * n_out * rb)
    fin = DeviceBuffer(gpu, n_out * _lib.PARTIAL_NBYTES)
    vbuf, kbuf = DeviceBuffer(gpu, n_out * 8), DeviceBuffer(gpu, n_out)
    engine.reduce_axes(gpu, plan.batch, plan.mask_up.struct, sum(1 << a for a in axes), mbuf.ptr, parts.ptr, st,
                       rec=rec)
    vals = np.ma.concatenate([_masked(chunks[c], MISS) for c in listed], axis=0)
    ex = exact_reference(vals, axes)
    for rtv in (True, False):
        engine.combine_segments(gpu, dt, parts.ptr, mbuf.ptr + 8 * 7, mbuf.ptr + 8 * (7 + index.size), n_out,
                                fin.ptr, rtv, st, rec=rec)
        final = np.zeros(n_out, dtype=engine.partial_dtype(dt))
        gpu.d2h(final, fin.ptr, st)
        gpu.synchronize(st)
        np.testing.assert_array_equal(final["count"], ex["n"])
        _note("combine_segments" + (" records" if rec else ""),
              assert_within(final["sum"], ex["exact"], sum_bound(dt, ex["n"], ex["abs_sum"]),
                            f"combine_segments rec={rec} round_to_var={rtv}"))
        engine.format_partials(gpu, dt, fin.ptr, n_out, "mean", vbuf.ptr, kbuf.ptr, None, st)
        means, mask = np.zeros(n_out, dtype=np.float64), np.zeros(n_out, dtype=np.bool_)
        gpu.d2h(means, vbuf.ptr, st)
        gpu.d2h(mask, kbuf.ptr, st)
        gpu.synchronize(st)
        assert not mask.any()
        _note("format_partials mean", assert_reduction_close(means, vals, axes, dt, "mean", f"format rec={rec}"))
    for b in (dbuf, mbuf, parts, fin, vbuf, kbuf):
        b.free()


# ---------------------------------------------------------------------------
# other paths
# ---------------------------------------------------------------------------
def test_resident_repeat_query(gpu, big):
    """Active(resident=True): the first query loads the chunks, the repeat is
    replayed from the cached plan; both hold the bound."""
    data, vals = big
    var = make_var(data, BIG_CHUNKS, ATTRS, shuffle=True)
    index = np.s_[0:16, 4:20, :]
    try:
        for method, axis in (("mean", None), ("sum", (0,)), ("mean", (0, 2))):
            for rep in range(3):
                a = Active(var, resident=True)
                getattr(a, method)(axis=axis)
                got = a[index]
                if rep:
                    assert a.data_read == 0
                ok = ~np.ma.getmaskarray(got).reshape(-1)
                _note(f"resident {'repeat' if rep else 'first'} query",
                      assert_reduction_close(got, vals[index], axis, "<f8", method,
                                             f"resident {method} {axis} rep {rep}", ok=ok))
    finally:
        release_resident(var)


def test_coalesced_reduce_chunk_under_a_thread_pool(gpu, tmp_path):
    """storage.reduce_chunk as the reference drives it (one call per chunk
    from a pool of threads, coalesced into batches on the device)."""
    rng = np.random.default_rng(81)
    shape = (8, 12, 32)
    arrs = [_data(rng, shape, dt, masked=True) for dt in ("<f8", ">f8") * 12]
    path = tmp_path / "chunks.bin"
    path.write_bytes(b"".join(a.tobytes() for a in arrs))
    sels = [np.s_[0:8, 0:12, 0:32], np.s_[2:7, 0:12, 0:32], np.s_[1:8:3, 0:12:2, 3:32:5]]
    jobs = [(k, sels[k % 3], axis, method) for k in range(len(arrs)) for axis in (None, (1,), (0, 2))
            for method in (np.ma.sum, np.ma.mean)]

    def one(job):
        k, sel, axis, method = job
        return pas.reduce_chunk(str(path), k * arrs[0].nbytes, arrs[0].nbytes, None, None, MISS, arrs[k].dtype.str,
                                shape, "C", sel, axis, method)

    before = gpu.coalescer_stats()
    with concurrent.futures.ThreadPoolExecutor(max_workers=30) as ex:
        res = list(ex.map(one, jobs))
    assert gpu.coalescer_stats()["chunks"] > before["chunks"]
    for (k, sel, axis, method), (got, gn) in zip(jobs, res):
        vals = _masked(arrs[k], MISS)[sel]
        kind = "mean" if method is np.ma.mean else "sum"
        np.testing.assert_array_equal(np.asarray(gn).reshape(-1), exact_reference(vals, axis)["n"])
        ok = ~np.ma.getmaskarray(got).reshape(-1)
        _note(f"coalesced reduce_chunk {kind}",
              assert_reduction_close(got, vals, axis, "<f8", kind, f"chunk {k} {sel} {axis} {kind}", ok=ok))


def test_sharded_total(gpu, big):
    """pyas_reduce_sharded over the devices visible (one is enough): every
    device ends with the same f64 total."""
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer, get_context
    from pyactivestorage_amd.distributed import equal_ranges
    data, vals = big
    nd = ctypes.c_int(0)
    _lib.check(gpu.lib.pyas_device_count(ctypes.byref(nd)), "pyas_device_count")
    ndev = max(1, min(nd.value, 2))
    blocks = [np.ascontiguousarray(data[tuple(slice(i * c, (i + 1) * c) for i, c in zip(cc, BIG_CHUNKS))])
              for cc in np.ndindex(5, 6, 10)]
    ctxs, plans, streams, keep = [], [], [], []
    for k, (lo, hi) in enumerate(equal_ranges(len(blocks), ndev)):
        c = get_context(k)
        st = c.thread_stream()
        blob = np.concatenate([np.frombuffer(b.tobytes(), np.uint8) for b in blocks[lo:hi]])
        d = DeviceBuffer(c, blob.nbytes)
        c.h2d(d.ptr, blob, st)
        c.synchronize(st)
        plans.append(ReductionPlan(c, np.dtype("<f8"), BIG_CHUNKS, d.ptr,
                                   np.arange(hi - lo, dtype=np.int64) * blocks[0].nbytes, missing=MISS, stream=st))
        ctxs.append(c)
        streams.append(st)
        keep.append(d)
    arr = lambda t, v: (t * len(v))(*v)  # noqa: E731
    outs = [DeviceBuffer(c, (ndev + 1) * _lib.PARTIAL_NBYTES) for c in ctxs]
    rc = gpu.lib.pyas_reduce_sharded(
        arr(ctypes.c_void_p, [c.handle for c in ctxs]),
        arr(ctypes.c_void_p, [ctypes.addressof(p.batch) for p in plans]),
        arr(ctypes.c_void_p, [ctypes.addressof(p.mask_up.struct) for p in plans]),
        ndev, 1, arr(ctypes.c_void_p, [o.ptr for o in outs]), arr(ctypes.c_void_p, streams))
    _lib.check(rc, "pyas_reduce_sharded")
    ex = exact_reference(vals)
    for c, o, s in zip(ctxs, outs, streams):
        host = np.zeros(ndev + 1, dtype=engine.partial_dtype(np.float64))
        c.d2h(host, o.ptr, s)
        c.synchronize(s)
        assert int(host[0]["count"]) == int(ex["n"][0])
        _note(f"sharded total (ndev={ndev})", assert_within(
            np.array([host[0]["sum"]]), ex["exact"], sum_bound("<f8", ex["n"], ex["abs_sum"]), "sharded"))


def test_reductionist_request(gpu, tmp_path):
    """One Reductionist sum request on a big-endian shuffled f8 object: the
    CBOR reply must carry float64."""
    import sys

    import requests

    from pyactivestorage_amd import reductionist_server as rs
    from tests.test_reductionist_wire import client_decode
    shape = (10, 12, 16)
    arr = _data(np.random.default_rng(17), shape, ">f8", masked=True)
    (tmp_path / "bucket").mkdir()
    (tmp_path / "bucket" / "v.bin").write_bytes(shuffle_bytes(arr, 8))
    srv = rs.ReductionistServer(str(tmp_path), ("127.0.0.1", 0))
    srv.start()
    try:
        for axis in (None, (0,), (1, 2)):
            body = {"interface_type": "s3", "url": "s3://bucket/v.bin", "dtype": "float64", "byte_order": "big",
                    "offset": 0, "size": arr.nbytes, "order": "C", "shape": list(shape),
                    "selection": [[1, 9, 2], [0, 12, 1], [3, 16, 4]],
                    "filters": [{"id": "shuffle", "element_size": 8}],
                    "missing": {"missing_value": FILL}}
            if axis is not None:
                body["axis"] = list(axis)
            r = requests.post(f"{srv.url}/v2/sum/", json=body, timeout=60)
            assert r.status_code == 200, r.text
            res, count = client_decode(r.content)
            assert np.asarray(res).dtype == np.float64, sys.byteorder
            vals = _masked(arr, rs.decode_missing({"missing_value": FILL}, arr.dtype))[1:9:2, 0:12:1, 3:16:4]
            ex = exact_reference(vals, axis)
            np.testing.assert_array_equal(np.asarray(count).reshape(-1), ex["n"])
            _note("Reductionist sum", assert_reduction_close(np.asarray(res), vals, axis, ">f8", "sum",
                                                             f"reductionist axis={axis}"))
    finally:
        srv.shutdown()
        srv.server_close()


def test_integer_mean(gpu):
    """<i8 mean at Active level: the i64 sum is exact, so the mean is within
    2 u |mean| of exact-integer-sum / count (the kernel's division and the
    reference's)."""
    rng = np.random.default_rng(64)
    shape, chunks = (20, 24, 16), (4, 4, 8)
    data = rng.integers(-2 ** 38, 2 ** 39, size=shape).astype("<i8")      # totals stay below 2**53
    data.reshape(-1)[rng.random(data.size) < 0.05] = -999
    var = make_var(data, chunks, {"_FillValue": np.array([-999], dtype="<i8")})
    keep = data != -999
    worst = 0.0
    for axis in (None, (0,), (1, 2)):
        a = Active(var)
        a.mean(axis=axis)
        got = a[...]
        assert got.dtype == np.float64
        ax = tuple(range(3)) if axis is None else axis
        kept = [d for d in range(3) if d not in ax]
        d2 = np.transpose(data, kept + list(ax)).reshape(int(np.prod([shape[d] for d in kept], dtype=int)), -1)
        k2 = np.transpose(keep, kept + list(ax)).reshape(d2.shape)
        g = np.ma.getdata(got).reshape(-1)
        assert not np.ma.getmaskarray(got).any()
        for j in range(d2.shape[0]):
            total = sum(int(v) for v in d2[j][k2[j]])          # Python ints: exact
            cnt = int(k2[j].sum())
            want = total / cnt                                 # correctly rounded int / int
            err = abs(float(g[j]) - want)
            assert err <= 2 * U64 * abs(want), (axis, j, g[j], want)
            worst = max(worst, err / (2 * U64 * abs(want)))
    _note("Active <i8 mean", worst)


def test_report_worst_ratios(gpu):
    """Per path, the worst observed |error| / bound of this module's run; a
    ratio above 1 has already failed its own test."""
    print("\nfloat64 accuracy, worst error/bound per path:")
    for path in sorted(RATIOS):
        print(f"  {path}: {RATIOS[path]:.3f}")
    assert all(r <= 1.0 for r in RATIOS.values())
