"""Host side of ``Active.trend``: the exported C entry points, ``trend.of`` /
``slope`` / ``intercept`` against ``np.polyfit``, the masking rules,
``trend.merge`` (``comoments.merge``) of a split selection, and the ``Active``
API checks that run before any device call."""
import ctypes

import numpy as np
import pytest

from pyactivestorage_amd import _lib, comoments, engine, trend
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


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pyas_trend_axes", "pyas_trend_cols", "pyas_trend_finalize"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2 and _lib.ABI_VERSION == 2
    assert ctypes.sizeof(_lib.Coord) == 24
    assert [(f[0], getattr(_lib.Coord, f[0]).offset) for f in _lib.Coord._fields_] == \
        [("pool", 0), ("origin", 8), ("dim", 16)]
    assert trend.merge is comoments.merge


def test_of_slope_intercept_match_polyfit():
    rng = np.random.default_rng(5)
    x = 6e4 + np.cumsum(rng.choice([28.0, 30.0, 31.0], 40))       # irregular, offset
    y = 0.02 * (x - 6e4) + rng.normal(0.0, 1.0, 40)
    ym = np.ma.MaskedArray(y, mask=rng.random(40) < 0.2)
    ok = ~ym.mask
    rec = trend.of(x, ym, 0)
    assert rec.dtype == engine.comoments_dtype and int(rec["count"]) == int(ok.sum())
    xc = x[ok] - x[ok].mean()
    b, a = np.polyfit(xc, y[ok], 1)                                # y = a + b (x - mean_x)
    np.testing.assert_allclose(trend.slope(rec), b, rtol=1e-12)
    np.testing.assert_allclose(trend.intercept(rec), a - b * x[ok].mean(), rtol=1e-12)
    np.testing.assert_allclose(rec["mean_x"], x[ok].mean(), rtol=1e-12)
    # broadcast along a middle dimension: every column sees the same coordinate
    y3 = np.ma.MaskedArray(np.broadcast_to(y[None, :, None], (2, 40, 3)).copy(),
                           mask=np.broadcast_to(ym.mask[None, :, None], (2, 40, 3)).copy())
    np.testing.assert_allclose(trend.slope(trend.of(x, y3, 1)), b, rtol=1e-12)
    np.testing.assert_allclose(trend.slope(trend.of(x, y3, -2)), b, rtol=1e-12)
    # integers convert as astype(float64) does; coord None is arange
    yi = (3 * np.arange(10) - 7).astype(np.int16)
    assert float(trend.slope(trend.of(None, yi, 0))) == 3.0
    assert float(trend.intercept(trend.of(None, yi, 0))) == -7.0
    with pytest.raises(ValueError):
        trend.of(x[:-1], ym, 0)
    with pytest.raises(ValueError):
        trend.of(x, ym, 1)


def test_masking_rules():
    x = np.array([1.0, 2.0, 4.0])
    y = np.ma.MaskedArray([3.0, 1.0, 2.0])
    none = np.ma.MaskedArray(y.data, mask=True)
    one = np.ma.MaskedArray(y.data, mask=[True, False, True])
    parts = np.concatenate([trend.of(x, y, 0).reshape(1), trend.of(x, one, 0).reshape(1),
                            trend.of(x, none, 0).reshape(1), trend.of(np.full(3, 2.5), y, 0).reshape(1),
                            trend.of(x, np.full(3, 7.25), 0).reshape(1)])
    assert parts["count"].tolist() == [3, 1, 0, 3, 3]
    for fn in (trend.slope, trend.intercept):
        got = fn(parts)
        assert got.dtype == np.float64 and got.shape == (5,)
        # n = 0 is masked; n = 1 and all-equal coordinates are 0/0: NaN, not masked
        assert np.ma.getmaskarray(got).tolist() == [False, False, True, False, False]
        assert np.isnan(got.data[1]) and np.isnan(got.data[3]) and not np.isnan(got.data[0])
    assert trend.slope(parts).data[4] == 0.0                      # constant data: exactly zero
    assert trend.intercept(parts).data[4] == 7.25
    # the components dict of a query is read like the records
    comp = {"n": parts["count"], **{k: np.ma.MaskedArray(parts[k], mask=parts["count"] == 0) for k in FIELDS[1:]}}
    assert trend.slope(comp).tobytes() == trend.slope(parts).tobytes()


def test_nan_stays_nan():
    x = np.arange(5.0)
    for bad in (np.nan, np.inf, -np.inf):
        y = np.array([1.0, 2.0, bad, 4.0, 5.0])
        rec = trend.of(x, y, 0)
        assert int(rec["count"]) == 5
        for fn in (trend.slope, trend.intercept):
            got = fn(rec)
            assert not np.ma.getmaskarray(got).any() and np.isnan(got.data).all()
    parts = comoments.records([3, 3], 1.0, 1.0, 2.0, [2.0, np.nan], [np.nan, np.nan])
    assert np.isnan(trend.slope(trend.merge(parts, parts)).data).all()


@pytest.mark.parametrize("cut", [0, 1, 500, 1000])
def test_merge_split(cut):
    rng = np.random.default_rng(11)
    x = 1.7e9 + 86400.0 * np.arange(1000)
    y = 288.0 + 2e-7 * (x - x[0]) + rng.normal(0.0, 5.0, 1000)
    ym = np.ma.MaskedArray(y, mask=rng.random(1000) < 0.1)
    whole = trend.of(x, ym, 0)
    a, b = trend.of(x[:cut], ym[:cut], 0), trend.of(x[cut:], ym[cut:], 0)
    got = trend.merge(a, b)
    assert got.dtype == engine.comoments_dtype and int(got["count"]) == int(whole["count"])
    for k in FIELDS[1:]:
        np.testing.assert_allclose(got[k], whole[k], rtol=1e-12, err_msg=k)
    np.testing.assert_allclose(trend.slope(got), trend.slope(whole), rtol=1e-12)
    np.testing.assert_allclose(trend.intercept(got), trend.intercept(whole), rtol=1e-12)


def test_check_coord():
    assert trend.check_coord(None, 4).tolist() == [0.0, 1.0, 2.0, 3.0]
    c = trend.check_coord([3, 1, 1, 2], 4)                         # repeats, not monotonic
    assert c.dtype == np.float64 and c.tolist() == [3.0, 1.0, 1.0, 2.0]
    for bad in ("abc", [1.0, "x", 2.0, 3.0], [[0.0, 1.0], [2.0, 3.0]], [0.0, 1.0, 2.0], 1.0,
                [0.0, np.nan, 2.0, 3.0], [0.0, 1.0, np.inf, 3.0], [None] * 4):
        with pytest.raises(ValueError):
            trend.check_coord(bad, 4)


# -- the Active API: every error before any device call --------------------------------
def test_api_returns_self_and_settings():
    a = Active(_var())
    assert a.trend_path is None
    assert a.trend(0) is a and a._method == "trend"
    assert a._trend["along"] == 0 and a._trend["coord"].tolist() == [0.0, 1.0]
    assert a.trend(-1, coord=[4, 3, 2, 1], axis=(2,)) is a
    assert a._trend["along"] == 2 and a._trend["coord"].tolist() == [4.0, 3.0, 2.0, 1.0] and a._axis == (2,)
    a.method = "mean"
    assert a._trend is None
    with pytest.raises(AttributeError):
        a.trend_path = "cols"


@pytest.mark.parametrize("along", [3, -4, True, 1.0, "0", None])
def test_bad_along(no_device, along):
    a = Active(_var())
    with pytest.raises(ValueError, match="along"):
        a.trend(along)
    assert a._method is None and a._trend is None


@pytest.mark.parametrize("coord", ["abc", [1.0, "x"], [[0.0, 1.0]], [0.0, 1.0, 2.0], 1.0, [0.0, np.nan],
                                   [np.inf, 1.0]])
def test_bad_coord(no_device, coord):
    a = Active(_var())
    with pytest.raises(ValueError, match="coord"):
        a.trend(0, coord=coord)
    assert a._method is None and a._trend is None


@pytest.mark.parametrize("along, axis", [(0, (1,)), (0, (1, 2)), (2, (0, 1)), (-1, 0)])
def test_along_must_be_reduced(no_device, along, axis):
    a = Active(_var())
    with pytest.raises(ValueError, match="not among the reduced axes"):
        a.trend(along, axis=axis)[...]
    assert a._method is None and a._trend is None              # the settings held for one query


def test_weights_are_refused(no_device):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.trend(0)[...]
    assert a._trend is None and a._weights is None and a._method is None


def test_group_not_implemented(no_device):
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="trend with group="):
        a.trend(0)[...]
    assert a._trend is None and a._method is None
