"""Host side of ``Active.cov`` / ``Active.corr``: the 48-byte
``pyas_comoments`` record in ctypes and NumPy, the exported C entry points,
``comoments.of`` / ``finalize_cov`` / ``finalize_corr`` against ``np.cov`` and
``np.corrcoef``, ``comoments.merge`` (Chan's formula with the cross term), and
the ``Active`` API checks that run before any device call."""
import ctypes

import numpy as np
import pytest

from pyactivestorage_amd import _lib, comoments, engine
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

FIELDS = ("count", "mean_x", "mean_y", "m2_x", "m2_y", "cxy")


def _var(dtype="<f4", shape=(2, 3, 4), chunks=None):
    data = np.arange(int(np.prod(shape))).astype(dtype).reshape(shape)
    chunks = chunks or shape
    raw = data.tobytes()
    return ChunkedVariable(name="v", shape=shape, chunks=chunks, dtype=np.dtype(dtype),
                           chunk_index={(0,) * len(shape): (0, len(raw))},
                           reader=lambda off, size: raw[off:off + size])


@pytest.fixture
def no_device(monkeypatch):
    from pyactivestorage_amd import active as mod

    def fail(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(mod, "get_context", fail)


def test_record_layout():
    assert ctypes.sizeof(_lib.Comoments) == 48 and _lib.COMOMENTS_NBYTES == 48
    dt = engine.comoments_dtype
    assert dt.itemsize == 48 and dt.names == FIELDS
    assert [dt.fields[k][1] for k in FIELDS] == [0, 8, 16, 24, 32, 40]
    assert [dt.fields[k][0] for k in FIELDS] == [np.dtype("<i8")] + [np.dtype("<f8")] * 5
    assert [(f[0], getattr(_lib.Comoments, f[0]).offset) for f in _lib.Comoments._fields_] == \
        list(zip(FIELDS, (0, 8, 16, 24, 32, 40)))


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pyas_comoments_axes", "pyas_comoments_combine_segments", "pyas_comoments_combine_grid"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2


@pytest.mark.parametrize("ddof", [0, 1])
def test_of_and_finalize_match_numpy(ddof):
    rng = np.random.default_rng(3)
    x = rng.normal(5.0, 2.0, 40)
    y = 0.3 * x + rng.normal(0.0, 1.0, 40)
    xm = np.ma.MaskedArray(x, mask=rng.random(40) < 0.2)
    ym = np.ma.MaskedArray(y, mask=rng.random(40) < 0.2)
    rec = comoments.of(xm, ym)
    ok = ~(xm.mask | ym.mask)
    assert rec.dtype == engine.comoments_dtype and int(rec["count"]) == int(ok.sum())
    np.testing.assert_allclose(comoments.finalize_cov(rec, ddof), np.cov(x[ok], y[ok], ddof=ddof)[0, 1], rtol=1e-12)
    np.testing.assert_allclose(comoments.finalize_corr(rec), np.corrcoef(x[ok], y[ok])[0, 1], rtol=1e-12)
    np.testing.assert_allclose(rec["m2_x"], x[ok].var() * ok.sum(), rtol=1e-12)
    np.testing.assert_allclose(rec["m2_y"], y[ok].var() * ok.sum(), rtol=1e-12)
    # integers convert as astype(float64) does
    xi = np.arange(10, dtype=np.int16)
    np.testing.assert_allclose(comoments.finalize_cov(comoments.of(xi, xi * xi)), np.cov(xi, xi * xi, ddof=0)[0, 1])
    with pytest.raises(ValueError):
        comoments.of(x, y[:-1])


def test_masking_rules():
    x, y = np.array([1.0, 2.0, 4.0]), np.array([3.0, 1.0, 2.0])
    parts = np.concatenate([comoments.of(x, y).reshape(1), comoments.of(x[:1], y[:1]).reshape(1),
                            comoments.of(x[:0], y[:0]).reshape(1), comoments.of(np.full(3, 2.5), y).reshape(1)])
    assert parts["count"].tolist() == [3, 1, 0, 3]
    for ddof in (0, 1):
        cov = comoments.finalize_cov(parts, ddof)
        assert cov.dtype == np.float64 and cov.shape == (4,)
        # n = 0 is masked; n = 1 is masked with ddof 1 and exactly 0 with ddof 0
        assert np.ma.getmaskarray(cov).tolist() == [False, ddof == 1, True, False]
        if ddof == 0:
            assert cov.data[1] == 0.0
        assert cov.data[3] == 0.0          # a constant side: exactly zero
    corr = comoments.finalize_corr(parts)
    assert corr.dtype == np.float64
    assert np.ma.getmaskarray(corr).tolist() == [False, False, True, False]
    # zero variance (one pair, or a constant side) is 0/0: NaN, not masked
    assert np.isnan(corr.data[1]) and np.isnan(corr.data[3]) and not np.isnan(corr.data[0])


def test_corr_is_clipped():
    parts = comoments.records([5, 5], 0.0, 0.0, 1.0, 1.0, [1.0 + 1e-15, -1.0 - 1e-15])
    assert comoments.finalize_corr(parts).data.tolist() == [1.0, -1.0]


def test_nan_stays_nan():
    parts = comoments.records([3, 3, 3], 1.0, 1.0, [np.nan, 2.0, 2.0], [2.0, np.nan, 2.0], [np.nan, np.nan, np.nan])
    for got in (comoments.finalize_cov(parts, 0), comoments.finalize_corr(parts)):
        assert not np.ma.getmaskarray(got).any()
        assert np.isnan(got.data).all()
    assert np.isnan(comoments.merge(parts, parts)["m2_x"][0])


@pytest.mark.parametrize("cut", [0, 1, 500, 1000])
def test_merge_split(cut):
    rng = np.random.default_rng(11)
    x = rng.normal(288.0, 10.0, 1000)
    y = -2.0 * x + rng.normal(0.0, 5.0, 1000)
    whole = comoments.of(x, y)
    a, b = comoments.of(x[:cut], y[:cut]), comoments.of(x[cut:], y[cut:])
    got = comoments.merge(a, b)
    assert got.dtype == engine.comoments_dtype
    assert int(got["count"]) == 1000
    for k in FIELDS[1:]:
        np.testing.assert_allclose(got[k], whole[k], rtol=1e-12, err_msg=k)
    if cut in (0, 1000):   # the empty side is neutral: the other side's bytes
        assert got.tobytes() == (b if cut == 0 else a).tobytes()
    empty = comoments.records(0, 0.0, 0.0, 0.0, 0.0, 0.0)
    assert comoments.merge(empty, empty).tobytes() == empty.tobytes()


def test_merge_broadcasts_elementwise():
    rng = np.random.default_rng(12)
    x, y = rng.normal(size=(4, 50)), rng.normal(size=(4, 50))
    a = np.concatenate([comoments.of(r[:20], s[:20]).reshape(1) for r, s in zip(x, y)])
    b = np.concatenate([comoments.of(r[20:], s[20:]).reshape(1) for r, s in zip(x, y)])
    want = np.concatenate([comoments.of(r, s).reshape(1) for r, s in zip(x, y)])
    got = comoments.merge(a, b)
    np.testing.assert_array_equal(got["count"], want["count"])
    np.testing.assert_allclose(got["cxy"], want["cxy"], rtol=1e-12, atol=1e-12)


# -- the Active API: every error before any device call --------------------------------
def test_api_methods_return_self():
    a, b = Active(_var()), Active(_var(">f4"))       # byte order may differ
    assert a.cov(b) is a and a._method == "cov" and a._ddof == 0 and a._co is b
    assert a.cov(a, axis=(0,), ddof=1) is a and a._ddof == 1 and a._axis == (0,) and a._co is a
    assert a.corr(b, axis=(1,)) is a and a._method == "corr" and a._ddof == 0 and a._axis == (1,)
    a.method = "mean"
    assert a._co is None


@pytest.mark.parametrize("method", ["cov", "corr"])
def test_argument_errors(no_device, method):
    a = Active(_var())
    call = getattr(a, method)
    for other in (None, _var(), np.zeros((2, 3, 4), "<f4")):
        with pytest.raises(TypeError):
            call(other)
    with pytest.raises(ValueError, match="shape"):
        call(Active(_var(shape=(2, 3, 5))))
    with pytest.raises(ValueError, match="chunk"):
        call(Active(_var(chunks=(2, 3, 2))))
    for dt in ("<f8", "<i4", "<u4"):       # item size or kind differs
        with pytest.raises(NotImplementedError, match="dtype"):
            call(Active(_var(dt)))
    with pytest.raises(ValueError, match="devices"):
        call(Active(_var(), device=1))
    assert a._method is None and a._co is None


@pytest.mark.parametrize("ddof", [-1, 1.5, True, "1"])
def test_bad_ddof(no_device, ddof):
    a = Active(_var())
    with pytest.raises(ValueError, match="ddof"):
        a.cov(a, ddof=ddof)


@pytest.mark.parametrize("method", ["cov", "corr"])
def test_weights_are_refused(no_device, method):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        getattr(a, method)(a)[...]
    assert a._co is None and a._weights is None      # the settings held for one query


@pytest.mark.parametrize("method", ["cov", "corr"])
@pytest.mark.parametrize("side", ["self", "other"])
def test_group_not_implemented(no_device, method, side):
    a = Active(_var(), group=object() if side == "self" else None)
    b = Active(_var(), group=object() if side == "other" else None)
    with pytest.raises(NotImplementedError, match="cov/corr with group="):
        getattr(a, method)(b)[...]
    assert a._co is None
