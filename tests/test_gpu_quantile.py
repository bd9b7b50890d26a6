"""``Active.quantile`` / ``.median`` on the device against ``np.quantile`` of
the float64 copy of the masked selection (taken with NumPy and masked with
``oracle.storage_ref.mask_missing``), per output.

Every comparison is ``==`` with equal NaNs; masks, dtype (float64) and shape
are compared too.  There are no tolerances.  ``n`` and ``nan`` of the
components are what the first pass's table rows sum to: they check the
per-pass invariant counts + below + above + nan == n.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import histogram as H
from pyactivestorage_amd import quantile as Q
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


def oracle(data, attrs, index, axis, q, method="linear"):
    """The components of the query: per output, np.quantile of the unmasked
    selection's float64 copy."""
    sel = np.ma.asarray(ref.mask_missing(data[index], get_missing_attributes(attrs or {})))
    nd = sel.ndim
    axes = tuple(range(nd)) if axis is None else tuple(a % nd for a in axis)
    kept = [d for d in range(nd) if d not in axes]
    final_shape = tuple(1 if d in axes else sel.shape[d] for d in range(nd))
    rows = np.ma.transpose(sel, kept + list(axes)).reshape(int(np.prod([sel.shape[d] for d in kept], dtype=np.int64)), -1)
    qs = np.asarray(q, dtype=np.float64)
    val = np.zeros((rows.shape[0],) + qs.shape, np.float64)
    n = np.zeros(rows.shape[0], np.int64)
    nan = np.zeros(rows.shape[0], np.int64)
    for r in range(rows.shape[0]):
        x = rows[r].compressed().astype(np.float64)
        n[r], nan[r] = x.size, np.isnan(x).sum()
        if x.size:
            with np.errstate(invalid="ignore"):
                val[r] = np.quantile(x, qs, method=method)
    mask = np.broadcast_to((n == 0).reshape((-1,) + (1,) * qs.ndim), val.shape)
    shape = final_shape + qs.shape
    return {"quantile": np.ma.MaskedArray(val.reshape(shape), mask=mask.reshape(shape)),
            "n": n.reshape(final_shape), "nan": nan.reshape(final_shape)}


def same_masked(got, want, what=""):
    assert isinstance(got, np.ma.MaskedArray), (what, type(got))
    assert got.dtype == np.float64 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    gm, wm = np.ma.getmaskarray(got), np.ma.getmaskarray(want)
    assert np.array_equal(gm, wm), what
    g, w = np.ma.getdata(got)[~gm], np.ma.getdata(want)[~wm]
    bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
    assert not bad.any(), (what, g[bad][:5], w[bad][:5])


def check(got, want, components, what=""):
    if not components:
        return same_masked(got, want["quantile"], what)
    assert isinstance(got, dict) and set(got) == {"quantile", "n", "nan"}, what
    same_masked(got["quantile"], want["quantile"], what)
    for k in ("n", "nan"):
        assert got[k].dtype == np.int64 and got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def query(var, q, axis, index, components=False, method="linear", stats=None):
    a = Active(var)
    a.components = components
    a.quantile(q, axis=axis, method=method)
    out = a[index]
    if stats is not None:
        stats.update(a._select_stats)
    return out


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
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
QS = [0, 0.25, 0.5, 0.95, 1]
FLT_MAX = np.finfo(np.float32).max


@functools.lru_cache(maxsize=None)
def spread_var(masked):
    """normal * 15 + 288 with -0.0, +0.0, a denormal and +-FLT_MAX planted;
    edge chunks padded with a value that would move every quantile."""
    rng = np.random.default_rng(200 + masked)
    data = (rng.normal(0.0, 1.0, SHAPE) * 15 + 288).astype("<f4")
    flat = data.reshape(-1)
    attrs, pad = {}, np.float32(-3.0e38)
    if masked:
        flat[rng.choice(flat.size, flat.size // 50, replace=False)] = -999.0
        outl = rng.choice(flat.size, 40, replace=False)
        flat[outl[:20]], flat[outl[20:]] = 150.0, 430.0            # beyond valid_min / valid_max
        one = lambda v: np.array([v], dtype="<f4")
        attrs = {"_FillValue": one(-999.0), "valid_min": one(200.0), "valid_max": one(380.0)}
        pad = np.float32(250.0)                                     # unmasked if it leaked
    plant = [-0.0, 0.0, 1e-40, FLT_MAX, -FLT_MAX]
    if masked:
        plant += [200.0, 380.0, 288.0, 288.0]                       # the valid range's ends (kept) and a tie
    plant = np.array(plant, dtype="<f4")
    flat[rng.choice(flat.size, plant.size, replace=False)] = plant
    data.setflags(write=False)
    return data, attrs, make_var(data, CHUNKS, attrs, pad=pad)


@functools.lru_cache(maxsize=None)
def spread_oracle(masked, iname, axis, method):
    data, attrs, _ = spread_var(masked)
    return oracle(data, attrs, NUMPY_INDEX.get(iname, dict(INDEXES)[iname]), axis, QS, method)


def _sweep_cases():
    for k, ((iname, index), axis, masked) in enumerate(itertools.product(INDEXES, AXES, (False, True))):
        comp = (k // 2) % 2 == 0
        yield pytest.param(iname, index, axis, masked, comp,
                           id=f"{iname}-{'all' if axis is None else ''.join(map(str, axis))}-"
                              f"{'masked' if masked else 'plain'}{'-comp' if comp else ''}")


@pytest.mark.parametrize("iname,index,axis,masked,comp", list(_sweep_cases()))
def test_sweep(gpu, iname, index, axis, masked, comp):
    _, _, var = spread_var(masked)
    check(query(var, QS, axis, index, comp), spread_oracle(masked, iname, axis, "linear"), comp)


@pytest.mark.parametrize("axis", [None, (1,)], ids=["all", "1"])
@pytest.mark.parametrize("method", Q.METHODS)
def test_every_method(gpu, method, axis):
    _, _, var = spread_var(True)
    qs = [0, 0.25, 0.5, 0.95, 1, 1 / 3, 0.505]
    data, attrs, _ = spread_var(True)
    want = oracle(data, attrs, dict(INDEXES)["inner"], axis, qs, method)
    check(query(var, qs, axis, dict(INDEXES)["inner"], True, method), want, True)


def test_scalar_q_and_median(gpu):
    data, attrs, var = spread_var(False)
    for axis in (None, (0, 2)):
        want = oracle(data, attrs, (Ellipsis,), axis, 0.5)
        assert want["quantile"].shape == tuple(1 if axis is None or d in axis else SHAPE[d] for d in range(3))
        same_masked(query(var, 0.5, axis, Ellipsis), want["quantile"])
        a = Active(var)
        a.median(axis=axis)
        same_masked(a[...], want["quantile"])


# -- 2. the prefix filter at every level -----------------------------------------------
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=["all", "0", "2"])
@pytest.mark.parametrize("dt", ["<f4", "<f8"])
def test_only_the_last_digit_decides(gpu, dt, axis):
    """f4: 288 + k 2^-15 (k < 1024) share the top 22 key bits; f8: 1 + k 2^-52
    share the top 54: every pass but the last finds one occupied digit."""
    rng = np.random.default_rng(11)
    k = rng.integers(0, 1024, (9, 14, 33))
    data = (288.0 + k * 2.0 ** -15).astype(dt) if dt == "<f4" else (1.0 + k * 2.0 ** -52).astype(dt)
    assert np.unique(data).size > 900
    keys = Q.keys(data.reshape(-1))
    assert np.unique(keys >> keys.dtype.type(10)).size == 1
    var = make_var(data, (4, 8, 16), pad=0)
    qs = [0, 0.1, 0.5, 0.77, 1]
    check(query(var, qs, axis, Ellipsis, True), oracle(data, None, (Ellipsis,), axis, qs), True)


# -- 3. ties -------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [None, (1,)], ids=["all", "1"])
def test_ties(gpu, axis):
    rng = np.random.default_rng(12)
    const = np.full((9, 14, 33), 271.5, "<f4")
    seven = rng.choice(np.array([-4.5, -1.0, 0.0, 0.25, 3.0, 3.5, 1e6], "<f4"), (9, 14, 33))
    for data in (const, seven):
        var = make_var(data, (4, 8, 16), pad=-7)
        for method in ("linear", "nearest"):
            check(query(var, QS, axis, Ellipsis, True, method), oracle(data, None, (Ellipsis,), axis, QS, method), True)


# -- 4. one chain or two ---------------------------------------------------------------
def test_median_chains(gpu):
    """An even count, half negative and half positive: the median's floor and
    ceil ranks lie in different first digits (the key flips at the sign), so
    two chains run.  With one element fewer the two ranks are one rank: one
    chain."""
    rng = np.random.default_rng(13)
    mag = rng.uniform(1.0, 100.0, 2 * 5 * 64).astype("<f4")
    mag[:320] *= -1
    data = rng.permutation(mag).reshape(2, 5, 64)
    var = make_var(data, (1, 5, 32))
    passes = len(Q.digits(32, Q.DIGIT_BITS))
    stats = {}
    same_masked(query(var, 0.5, None, Ellipsis, stats=stats), oracle(data, None, (Ellipsis,), None, 0.5)["quantile"])
    assert stats["chains"] == 2 and stats["passes"] == 1 + 2 * (passes - 1), stats
    med = float(np.median(data.astype(np.float64)))
    assert np.sort(data.reshape(-1))[319] < 0 < np.sort(data.reshape(-1))[320] and abs(med) < 100
    index = (slice(0, 1), slice(None), slice(0, 63))             # 315 elements: an odd count
    stats = {}
    same_masked(query(var, 0.5, None, index, stats=stats), oracle(data, None, index, None, 0.5)["quantile"])
    assert stats["chains"] == 1 and stats["passes"] == passes, stats


# -- 5. dtypes -----------------------------------------------------------------------
def dtype_data(dt):
    dt = np.dtype(dt)
    rng = np.random.default_rng(14)
    shape = (9, 14, 33)
    if dt.kind == "f":
        data = rng.normal(0.0, 40.0, shape).astype(dt)
    elif dt == np.dtype("<i2"):
        data = rng.integers(-3000, 3000, shape).astype(dt)
    elif dt == np.dtype("|u1"):
        data = rng.integers(0, 256, shape).astype(dt)
    elif dt == np.dtype("<i8"):
        data = rng.choice(np.array([2 ** 53 + 1, 2 ** 53, 2 ** 53 + 3, -(2 ** 53) - 1, -(2 ** 53) - 3, 5, -5,
                                    2 ** 62, -(2 ** 62)], dtype=np.int64), shape).astype(dt)
    else:   # <u8
        data = (rng.integers(0, 2 ** 62, shape, dtype=np.uint64) + np.uint64(2 ** 63)).astype(dt)
        data.reshape(-1)[:3] = [2 ** 64 - 1, 2 ** 63 - 1, 2 ** 63 + 2 ** 11 + 1]
    return data


# each stored plain and byte-shuffled (a 1-byte type has no byte shuffle)
@pytest.mark.parametrize("dt,shuffle", [(dt, sh) for dt in [">f4", "<f8", "<i2", "|u1", "<i8", "<u8"]
                                        for sh in (False, True) if not (sh and np.dtype(dt).itemsize == 1)],
                         ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v) if isinstance(v, bool) else v[1:])
def test_dtypes(gpu, dt, shuffle):
    data = dtype_data(dt)
    var = make_var(data, (4, 8, 16), shuffle=shuffle, pad=1)
    for axis, method in ((None, "linear"), ((1,), "lower"), ((2,), "midpoint")):
        check(query(var, QS, axis, Ellipsis, True, method), oracle(data, None, (Ellipsis,), axis, QS, method), True,
              (dt, axis))


# -- 6. NaN and infinities ---------------------------------------------------------------
def test_nan_rows_are_nan(gpu):
    rng = np.random.default_rng(15)
    data = rng.normal(0.0, 2.0, (9, 14, 33)).astype("<f4")
    data[1, 3, 5] = data[1, 9, 5] = data[7, 0, 32] = np.nan
    var = make_var(data, (4, 8, 16), pad=np.nan)
    for axis in ((1,), (0, 1), None):
        want = oracle(data, None, (Ellipsis,), axis, QS)
        got = query(var, QS, axis, Ellipsis, True)
        check(got, want, True, axis)
        nan_rows = got["nan"] > 0
        assert np.isnan(np.ma.getdata(got["quantile"])[nan_rows]).all()
        assert not np.isnan(np.ma.getdata(got["quantile"])[~nan_rows]).any()
        assert int(got["nan"].sum()) == 3


def test_infinities(gpu):
    rng = np.random.default_rng(16)
    data = rng.normal(0.0, 2.0, (9, 14, 33)).astype("<f4")
    pos = rng.choice(data.size, 60, replace=False)
    data.reshape(-1)[pos[:30]] = np.inf
    data.reshape(-1)[pos[30:]] = -np.inf
    data[0, 0, :] = np.inf                                        # a row of +inf only
    var = make_var(data, (4, 8, 16))
    for axis in (None, (2,)):
        for method, qs in (("lower", [0, 1]), ("higher", [0, 1]), ("linear", QS)):
            check(query(var, qs, axis, Ellipsis, True, method), oracle(data, None, (Ellipsis,), axis, qs, method), True,
                  (axis, method))


# -- 7. masked outputs -------------------------------------------------------------------
def test_all_fill_row_is_masked(gpu):
    rng = np.random.default_rng(17)
    data = rng.normal(10.0, 2.0, (9, 14, 33)).astype("<f4")
    data[:, 4, :] = -999.0
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    var = make_var(data, (4, 8, 16), attrs, pad=-999.0)
    got = query(var, QS, (2,), Ellipsis, True)
    check(got, oracle(data, attrs, (Ellipsis,), (2,), QS), True)
    assert np.ma.getmaskarray(got["quantile"])[:, 4].all() and not got["n"][:, 4].any()
    assert not np.ma.getmaskarray(got["quantile"])[:, 3].any()


# -- 8 and 9. digit widths and the table cap -----------------------------------------------
@pytest.mark.parametrize("bits", [3, 8, 11])
def test_digit_widths_agree(gpu, monkeypatch, bits):
    data, attrs, var = spread_var(True)
    monkeypatch.setattr(Q, "DIGIT_BITS", bits)
    for axis in ((0,), (2,), None):
        stats = {}
        got = query(var, QS, axis, dict(INDEXES)["stride"], stats=stats)
        same_masked(got, spread_oracle(True, "stride", axis, "linear")["quantile"], (bits, axis))
        assert stats["bits"] == bits


def test_cap_narrows_the_digits(gpu, monkeypatch):
    data, attrs, var = spread_var(False)
    n_out = SHAPE[0] * SHAPE[1]
    monkeypatch.setattr(H, "TABLE_CAP_BYTES", n_out * ((1 << 5) + 3) * 8)     # room for 5-bit digits, not 6
    stats = {}
    same_masked(query(var, QS, (2,), Ellipsis, stats=stats), spread_oracle(False, "all", (2,), "linear")["quantile"])
    assert stats["bits"] == 5 < Q.DIGIT_BITS


# -- 10. determinism ---------------------------------------------------------------------
def test_same_bytes_twice(gpu):
    _, _, var = spread_var(True)
    for axis in (None, (1,)):
        a, b = (query(var, QS, axis, Ellipsis, True) for _ in range(2))
        for k in ("quantile", "n", "nan"):
            assert np.ma.getdata(a[k]).tobytes() == np.ma.getdata(b[k]).tobytes()
        assert np.array_equal(np.ma.getmaskarray(a["quantile"]), np.ma.getmaskarray(b["quantile"]))


# -- 11. branches the shapes above do not reach (the cases of tests/_stats_gaps.py) -----------
from tests import _stats_gaps as G   # noqa: E402

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
    check(query(var, G.QS, axis, index, True), oracle(data, attrs, index, axis, G.QS), True,
          f"{group} {name} {dt} {iname} {G.axis_id(axis)}")


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(gpu, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in its launch."""
    data, attrs, var = gap_var("G2", name, "<f4", masked)
    k = G.G2_SECOND_TRIP
    want = oracle(data, attrs, (Ellipsis,), (0,), G.QS)
    got = query(var, G.QS, (0,), Ellipsis, True)
    what = f"G2 {name}: the second trip, outputs {k}..16899"
    for key in ("n", "nan"):
        assert np.array_equal(got[key].reshape(-1)[k:], want[key].reshape(-1)[k:]), (what, key)
    same_masked(got["quantile"].reshape(-1, len(G.QS))[k:], want["quantile"].reshape(-1, len(G.QS))[k:], what)
    check(got, want, True, f"G2 {name}: every output")


@MASKED
@pytest.mark.parametrize("iname", ["whole", "from1"])
@pytest.mark.parametrize("axis", [None, (0,), (2,)], ids=G.axis_id)
@pytest.mark.parametrize("dt", G.G3_DTYPES)
def test_g3_shuffled_chunks_of_odd_size(gpu, dt, axis, iname, masked):
    """Shuffled chunks of 105 elements: hist_run_shuffled's per-element
    fallback under the digit counts."""
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


# (test_dtypes has <u8, and >f4 for a swapped type: the types it leaves out)
@MASKED
@pytest.mark.parametrize("dt,shuffle", [(dt, sh) for dt, sh in G.G5_LAYOUTS if dt != "<u8"],
                         ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    for axis in (None, (1,)):
        gap_check("G5", "dtypes", dt, masked, "whole", axis, shuffle)


@pytest.mark.parametrize("dt,off", G.G6_CASES)
def test_g6_base_misaligned(gpu, dt, off):
    """One chunk ``off`` bytes into its buffer, every dim reduced, through
    pyas_select_axes itself: the key's first digit, then a digit below it
    under a prefix (f4: the fullest first digit's next 8 bits; u1, whose key
    is the value: the last 8 bits), against the counts of quantile.keys."""
    from pyactivestorage_amd import engine
    from pyactivestorage_amd.device import DeviceBuffer
    data = G.g6_chunk(dt, spread=True)
    for iname, index in G.G6_INDEXES.items():
        st, buf, plan = G.misaligned_plan(gpu, data, off, index)
        keys = Q.keys(data[Ellipsis if index is None else index].reshape(-1)).astype(np.uint64)
        first = np.bincount((keys >> np.uint64(24)).astype(np.int64), minlength=256)
        top = int(first.argmax())
        shift = 16 if dt == "<f4" else 0
        assert (first > 0).sum() >= (8 if dt == "<f4" else 1) and first[top] > 256
        tbuf, pbuf = DeviceBuffer(gpu, (256 + 3) * 8), DeviceBuffer(gpu, 16)
        gpu.h2d(pbuf.ptr, np.array([top, 0], np.uint64), st)
        for prefix_ptr, sh in ((None, 24), (pbuf.ptr, shift)):
            engine.hist_reset(gpu, tbuf.ptr, 1, 256, st)
            engine.select_axes(gpu, plan.batch, plan.mask_up.struct, prefix_ptr, sh, 8, 0b111, None, None, tbuf.ptr, st)
            tab = np.full(256 + 3, -1, np.int64)
            gpu.d2h(tab, tbuf.ptr, st)
            gpu.synchronize(st)
            want = np.zeros(256 + 3, np.int64)
            if prefix_ptr is None:
                want[:256] = first
            else:
                hi = keys >> np.uint64(sh + 8)
                on = hi == np.uint64(top)
                want[:256] = np.bincount(((keys[on] >> np.uint64(sh)) & np.uint64(255)).astype(np.int64), minlength=256)
                want[256], want[257] = (hi < np.uint64(top)).sum(), (hi > np.uint64(top)).sum()
                assert (want[:256] > 0).sum() > 100
            assert np.array_equal(tab, want), (f"G6 {dt} offset {off} {iname} shift {sh}", tab, want)
