"""Host side of ``Active.var`` / ``std`` / ``cov`` / ``corr`` with
``weights=``: the 64-byte ``pyas_wcomoments`` record in ctypes, NumPy and the
header, the exported C entry points, ``wmoments.of`` / ``merge`` /
``finalize_*`` against a brute-force two-pass NumPy and ``np.cov(aweights=)``,
and the ``Active`` API checks that run before any device call."""
import ctypes
import os
import re

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, wmoments
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("count", "sw", "sw2", "mean_x", "mean_y", "m2_x", "m2_y", "cxy")
ENTRY_POINTS = ("pyas_wcomoments_axes", "pyas_wcomoments_combine_segments", "pyas_wcomoments_combine_grid")
EMPTY = wmoments.records(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


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


W = {0: [1.0, 2.0], 2: [0.5, 0.0, 1.5, 1.0]}


def _call(a, method, **kw):
    """``a.var(**kw)`` ... ``a.corr(a, **kw)`` (corr takes no ddof)."""
    if method in ("var", "std"):
        return getattr(a, method)(**kw)
    if method == "corr":
        kw.pop("ddof", None)
    return getattr(a, method)(a, **kw)


# -- the record and the library ---------------------------------------------------------------
def test_record_layout_matches_the_header():
    assert ctypes.sizeof(_lib.Wcomoments) == 64 and _lib.WCOMOMENTS_NBYTES == 64
    dt = engine.wcomoments_dtype
    assert dt.itemsize == 64 and dt.names == FIELDS
    assert [dt.fields[k][1] for k in FIELDS] == [8 * i for i in range(8)]
    assert [dt.fields[k][0] for k in FIELDS] == [np.dtype("<i8")] + [np.dtype("<f8")] * 7
    assert [(f[0], getattr(_lib.Wcomoments, f[0]).offset) for f in _lib.Wcomoments._fields_] == \
        [(name, 8 * i) for i, name in enumerate(FIELDS)]
    with open(os.path.join(ROOT, "include", "pyas.h")) as f:
        text = f.read()
    body = re.search(r"typedef struct \{([^}]*)\} pyas_wcomoments;", text).group(1)
    decl = [(m.group(1), [n.strip() for n in m.group(2).split(",")])
            for m in re.finditer(r"(int64_t|double)\s+([^;]+);", body)]
    assert decl == [("int64_t", ["count"]), ("double", list(FIELDS[1:]))]   # 8 fields of 8 bytes, in this order
    assert re.search(r"#define PYAS_ABI_VERSION\s+2\b", text)


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2


# -- of / merge / finalize ----------------------------------------------------------------------
def _brute(x, w, y=None):
    """Two passes in plain NumPy over the compressed float64 values."""
    sw, sw2 = w.sum(), (w * w).sum()
    mx = (w * x).sum() / sw
    out = {"sw": sw, "sw2": sw2, "mean_x": mx, "m2_x": (w * (x - mx) ** 2).sum()}
    if y is not None:
        my = (w * y).sum() / sw
        out.update(mean_y=my, m2_y=(w * (y - my) ** 2).sum(), cxy=(w * (x - mx) * (y - my)).sum())
    return out


@pytest.mark.parametrize("ddof", [0, 1])
def test_of_and_finalize_match_numpy(ddof):
    rng = np.random.default_rng(3)
    x = rng.normal(5.0, 2.0, 40)
    y = 0.3 * x + rng.normal(0.0, 1.0, 40)
    w = rng.uniform(0.1, 2.0, 40)
    w[[3, 17]] = 0.0
    xm = np.ma.MaskedArray(x, mask=rng.random(40) < 0.2)
    ym = np.ma.MaskedArray(y, mask=rng.random(40) < 0.2)
    ok = ~(xm.mask | ym.mask)
    rec = wmoments.of(xm, w, ym)
    assert rec.dtype == engine.wcomoments_dtype and int(rec["count"]) == int(ok.sum())
    for k, v in _brute(x[ok], w[ok], y[ok]).items():
        np.testing.assert_allclose(rec[k], v, rtol=1e-12, err_msg=k)
    c = np.cov(x[ok], y[ok], aweights=w[ok], ddof=ddof)
    np.testing.assert_allclose(wmoments.finalize_cov(rec, ddof), c[0, 1], rtol=1e-12)
    np.testing.assert_allclose(wmoments.finalize_var(rec, ddof), c[0, 0], rtol=1e-12)
    np.testing.assert_allclose(wmoments.finalize_var(rec, ddof, std=True), np.sqrt(c[0, 0]), rtol=1e-12)
    np.testing.assert_allclose(wmoments.finalize_corr(rec), c[0, 1] / np.sqrt(c[0, 0] * c[1, 1]), rtol=1e-12)
    # one variable: the y fields stay 0, the x fields are the same
    one = wmoments.of(np.ma.MaskedArray(x, mask=~ok), w)
    assert float(one["mean_y"]) == 0.0 and float(one["m2_y"]) == 0.0 and float(one["cxy"]) == 0.0
    for k in ("count", "sw", "sw2", "mean_x", "m2_x"):
        assert one[k] == rec[k], k
    # integers convert as astype(float64) does; the weights broadcast
    xi = np.arange(12, dtype=np.int16).reshape(3, 4)
    wi = np.array([1.0, 2.0, 0.5, 3.0])
    np.testing.assert_allclose(wmoments.finalize_var(wmoments.of(xi, wi)),
                               np.cov(xi.reshape(-1), aweights=np.tile(wi, 3), ddof=0), rtol=1e-12)
    with pytest.raises(ValueError):
        wmoments.of(x, w, y[:-1])


@pytest.mark.parametrize("cut", [0, 1, 500, 1000])
def test_merge_split(cut):
    rng = np.random.default_rng(11)
    x = rng.normal(288.0, 10.0, 1000)
    y = -2.0 * x + rng.normal(0.0, 5.0, 1000)
    w = rng.uniform(0.0, 3.0, 1000)
    whole = wmoments.of(x, w, y)
    a, b = wmoments.of(x[:cut], w[:cut], y[:cut]), wmoments.of(x[cut:], w[cut:], y[cut:])
    got = wmoments.merge(a, b)
    assert got.dtype == engine.wcomoments_dtype and int(got["count"]) == 1000
    for k in FIELDS[1:]:
        np.testing.assert_allclose(got[k], whole[k], rtol=1e-12, err_msg=k)
    if cut in (0, 1000):   # the empty record is neutral in both orders: the other side's bytes
        assert got.tobytes() == (b if cut == 0 else a).tobytes()


def test_merge_is_neutral_on_the_empty_record():
    rec = wmoments.of(np.array([1.0, 2.0, 4.0]), np.array([0.5, 1.0, 2.0]), np.array([3.0, 1.0, 2.0]))
    assert wmoments.merge(EMPTY, rec).tobytes() == rec.tobytes()
    assert wmoments.merge(rec, EMPTY).tobytes() == rec.tobytes()
    assert wmoments.merge(EMPTY, EMPTY).tobytes() == EMPTY.tobytes()
    assert EMPTY.tobytes() == bytes(64)


def test_merge_broadcasts_elementwise():
    rng = np.random.default_rng(12)
    x, y, w = rng.normal(size=(4, 50)), rng.normal(size=(4, 50)), rng.uniform(0.1, 2.0, (4, 50))
    parts = lambda lo, hi: np.concatenate([wmoments.of(r[lo:hi], v[lo:hi], s[lo:hi]).reshape(1)
                                           for r, s, v in zip(x, y, w)])
    got, want = wmoments.merge(parts(0, 20), parts(20, 50)), parts(0, 50)
    np.testing.assert_array_equal(got["count"], want["count"])
    for k in FIELDS[1:]:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=1e-12, err_msg=k)


def test_a_zero_weight_side_adds_its_count_and_its_nan():
    x, y = np.array([1.0, 2.0, 4.0]), np.array([3.0, 1.0, 2.0])
    a = wmoments.of(x, np.array([0.5, 1.0, 2.0]), y)
    zero = wmoments.of(np.array([7.0, 9.0]), np.zeros(2), np.array([1.0, 5.0]))
    assert int(zero["count"]) == 2 and float(zero["sw"]) == 0.0 and float(zero["mean_x"]) == 0.0
    assert float(zero["m2_x"]) == 0.0 and float(zero["cxy"]) == 0.0
    for got in (wmoments.merge(a, zero), wmoments.merge(zero, a)):
        assert int(got["count"]) == 5
        for k in FIELDS[1:]:           # no mean from the weightless side: the other side's fields, exactly
            assert got[k] == a[k], k
    nan = wmoments.of(np.array([7.0, np.nan]), np.zeros(2), np.array([1.0, 5.0]))
    assert np.isnan(nan["m2_x"]) and np.isnan(nan["cxy"]) and float(nan["m2_y"]) == 0.0
    for got in (wmoments.merge(a, nan), wmoments.merge(nan, a)):
        assert int(got["count"]) == 5 and got["sw"] == a["sw"] and got["mean_x"] == a["mean_x"]
        assert np.isnan(got["m2_x"]) and np.isnan(got["cxy"]) and got["m2_y"] == a["m2_y"]
        assert np.isnan(wmoments.finalize_var(got).data) and not np.ma.getmaskarray(wmoments.finalize_var(got))
        assert np.isnan(wmoments.finalize_cov(got).data) and np.isnan(wmoments.finalize_corr(got).data)
    inf = wmoments.of(np.array([np.inf]), np.zeros(1))
    assert np.isnan(inf["m2_x"])


def test_masking_rules():
    x, y = np.array([1.0, 2.0, 4.0]), np.array([3.0, 1.0, 2.0])
    one_w = np.array([0.0, 0.7, 0.0])
    parts = np.concatenate([r.reshape(1) for r in (
        wmoments.of(x, np.array([0.5, 1.0, 2.0]), y),      # three weights
        wmoments.of(x, one_w, y),                          # exactly one positive weight
        wmoments.of(x, np.zeros(3), y),                    # every weight 0
        EMPTY.reshape(()),                                 # nothing counted
        wmoments.of(np.full(3, 2.5), np.array([0.5, 1.0, 2.0]), y))])   # a constant side
    assert parts["count"].tolist() == [3, 3, 3, 0, 3]
    for ddof in (0, 1):
        for got in (wmoments.finalize_var(parts, ddof), wmoments.finalize_var(parts, ddof, std=True),
                    wmoments.finalize_cov(parts, ddof)):
            assert got.dtype == np.float64 and got.shape == (5,)
            # sw == 0 is masked; one positive weight is masked with ddof 1 (sw sw - sw2 is exactly 0)
            assert np.ma.getmaskarray(got).tolist() == [False, ddof == 1, True, True, False]
            if ddof == 0:
                assert got.data[1] == 0.0
            assert got.data[4] == 0.0          # a constant side: exactly zero
    corr = wmoments.finalize_corr(parts)
    assert np.ma.getmaskarray(corr).tolist() == [False, False, True, True, False]
    assert np.isnan(corr.data[1]) and np.isnan(corr.data[4]) and not np.isnan(corr.data[0])


def test_corr_is_clipped():
    parts = wmoments.records([5, 5], 2.0, 1.0, 0.0, 0.0, 1.0, 1.0, [1.0 + 1e-15, -1.0 - 1e-15])
    assert wmoments.finalize_corr(parts).data.tolist() == [1.0, -1.0]


# -- the Active API: every error before any device call --------------------------------------------
@pytest.mark.parametrize("method", ["var", "std", "cov", "corr"])
def test_api_methods_return_self(method):
    a = Active(_var())
    assert _call(a, method, weights=W) is a and a._method == method
    assert sorted(a._mweights) == [0, 2] and a._mweights[2].dtype == np.float64
    assert a._weights is None and a.weights is None      # the property belongs to mean / sum
    assert _call(a, method) is a and a._mweights is None  # the keyword is per call
    _call(a, method, weights={-1: W[2]}, axis=(0,), ddof=1)
    assert sorted(a._mweights) == [2] and a._axis == (0,) and a._ddof == (0 if method == "corr" else 1)
    a.method = "mean"
    assert a._mweights is None


@pytest.mark.parametrize("method", ["var", "std", "cov", "corr"])
def test_argument_errors(no_device, method):
    a = Active(_var())
    for bad, word in (({3: [1.0]}, "out of range"), ({-4: [1.0]}, "out of range"), ({True: [1.0, 1.0]}, "out of range"),
                      ({0: [1.0, 2.0, 3.0]}, "2 entries"), ({2: [[1.0, 2.0, 3.0, 4.0]]}, "4 entries"),
                      ({0: [1.0, -2.0]}, "negative"), ({0: [1.0, np.nan]}, "NaN"), ({0: [1.0, np.inf]}, "infinite"),
                      ({0: [1.0, 2.0], -3: [1.0, 2.0]}, "twice"), ({0: ["a", "b"]}, "not numeric"),
                      ([1.0, 2.0], "mapping"), (np.ones(2), "mapping")):
        with pytest.raises(ValueError, match=word):
            _call(a, method, weights=bad)
    assert a._method is None and a._mweights is None


@pytest.mark.parametrize("method", ["var", "std", "cov", "corr"])
def test_settings_hold_for_one_query(no_device, method):
    """A query that fails before any device call (an index that drops an axis)
    still clears the keyword's slot."""
    a = Active(_var())
    _call(a, method, weights=W)
    with pytest.raises(IndexError):
        a[0]
    assert a._mweights is None and a._method is None and a._co is None


@pytest.mark.parametrize("method", ["var", "std", "cov", "corr"])
def test_the_weights_property_is_still_refused(no_device, method):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        _call(a, method, weights=W)[...]
    assert a._weights is None and a._mweights is None
    a.mean(weights={0: [1.0, 2.0]})
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        _call(a, method, weights=W)[...]


@pytest.mark.parametrize("method", ["var", "std", "cov", "corr"])
def test_group_not_implemented_comes_first(no_device, method):
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="cov/corr with group=" if method in ("cov", "corr")
                       else "var/std with group="):
        _call(a, method, weights=W)[...]
    assert a._mweights is None


def test_a_plain_mean_after_a_weighted_var_is_unweighted(monkeypatch):
    """``var(weights=W)[...]`` then ``mean()[...]``: the second query carries no
    weights of either kind into its reduction."""
    a = Active(_var())
    seen = []
    monkeypatch.setattr(Active, "_reduce_wmoments",
                        lambda self, *args: seen.append(("wmoments", dict(self._mweights), self._weights)) or "w")
    monkeypatch.setattr(Active, "_reduce", lambda self, *args: seen.append(("plain", self._mweights, self._weights)))
    monkeypatch.setattr(Active, "_reduce_weighted", lambda self, *args: seen.append(("weighted",)))
    assert a.var(weights=W)[...] == "w"
    a.mean()[...]
    assert [s[0] for s in seen] == ["wmoments", "plain"]
    assert sorted(seen[0][1]) == [0, 2] and seen[0][2] is None
    assert seen[1][1] is None and seen[1][2] is None
