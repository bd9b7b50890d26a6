"""Host side of ``Active.var`` / ``Active.std``: the 32-byte ``pyas_moments``
record in ctypes and NumPy, the exported C entry points, ``moments.finalize``
against ``np.ma.var`` / ``np.ma.std``, ``moments.merge`` (Chan's formula),
and the ``Active`` API checks that run before any device call."""
import ctypes

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, moments
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable


def _var():
    data = np.arange(24, dtype="<f4").reshape(2, 3, 4)
    raw = data.tobytes()
    return ChunkedVariable(name="v", shape=data.shape, chunks=data.shape, dtype=np.dtype("<f4"),
                           chunk_index={(0, 0, 0): (0, len(raw))}, reader=lambda off, size: raw[off:off + size])


def test_record_layout():
    assert ctypes.sizeof(_lib.Moments) == 32
    dt = engine.moments_dtype
    assert dt.itemsize == 32
    assert [dt.fields[k][1] for k in ("count", "mean", "m2")] == [0, 8, 16]
    assert [dt.fields[k][0] for k in ("count", "mean", "m2")] == [np.dtype("<i8"), np.dtype("<f8"), np.dtype("<f8")]
    assert [(f[0], getattr(_lib.Moments, f[0]).offset) for f in _lib.Moments._fields_[:3]] == \
        [("count", 0), ("mean", 8), ("m2", 16)]


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pyas_moments_axes", "pyas_moments_combine_segments", "pyas_moments_combine_grid"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2


@pytest.mark.parametrize("std", [False, True])
@pytest.mark.parametrize("ddof", [0, 1])
def test_finalize_matches_np_ma(ddof, std):
    rng = np.random.default_rng(3)
    rows = [rng.normal(5.0, 2.0, 7), rng.normal(-1.0, 0.1, 2), np.array([4.25]), np.zeros(0)]
    parts = np.concatenate([moments.of(r).reshape(1) for r in rows])
    assert parts["count"].tolist() == [7, 2, 1, 0]
    got = moments.finalize(parts, ddof, std)
    assert got.dtype == np.float64 and got.shape == (4,)
    # count 0 is masked; count 1 is masked with ddof 1 and exactly 0 with ddof 0
    assert np.ma.getmaskarray(got).tolist() == [False, False, ddof == 1, True]
    fn = np.ma.std if std else np.ma.var
    for k, r in enumerate(rows[:2] + ([rows[2]] if ddof == 0 else [])):
        want = fn(np.ma.MaskedArray(r, mask=np.zeros(r.size, bool)), ddof=ddof)
        np.testing.assert_allclose(got[k], want, rtol=1e-12)
    if ddof == 0:
        assert got.data[2] == 0.0
    for k, r in enumerate(rows):   # np.ma agrees on which results are masked
        full = np.ma.MaskedArray(np.append(r, 0.0), mask=np.append(np.zeros(r.size, bool), True))
        assert bool(np.ma.getmaskarray(fn(full, ddof=ddof))) == bool(np.ma.getmaskarray(got)[k])


def test_finalize_nan_m2_stays_nan():
    parts = moments.records([3, 3], [1.0, np.nan], [np.nan, np.nan])
    for std in (False, True):
        got = moments.finalize(parts, 0, std)
        assert not np.ma.getmaskarray(got).any()
        assert np.isnan(got.data).all()


@pytest.mark.parametrize("cut", [0, 1, 500, 1000])
def test_merge_split(cut):
    x = np.random.default_rng(11).normal(288.0, 10.0, 1000)
    whole = moments.of(x)
    a, b = moments.of(x[:cut]), moments.of(x[cut:])
    got = moments.merge(a, b)
    assert got.dtype == engine.moments_dtype
    assert int(got["count"]) == 1000
    np.testing.assert_allclose(got["mean"], whole["mean"], rtol=1e-12)
    np.testing.assert_allclose(got["m2"], whole["m2"], rtol=1e-12)
    if cut in (0, 1000):   # the empty side is neutral: the other side's bytes
        assert got.tobytes() == (b if cut == 0 else a).tobytes()
    empty = moments.records(0, 0.0, 0.0)
    assert moments.merge(empty, empty).tobytes() == empty.tobytes()


def test_merge_broadcasts_elementwise():
    x = np.random.default_rng(12).normal(size=(4, 50))
    a = np.concatenate([moments.of(r[:20]).reshape(1) for r in x])
    b = np.concatenate([moments.of(r[20:]).reshape(1) for r in x])
    got = moments.merge(a, b)
    want = np.concatenate([moments.of(r).reshape(1) for r in x])
    np.testing.assert_allclose(got["m2"], want["m2"], rtol=1e-12)
    np.testing.assert_array_equal(got["count"], want["count"])


def test_api_methods_return_self():
    a = Active(_var())
    assert a.var() is a and a._method == "var" and a._ddof == 0
    assert a.std(axis=(0,), ddof=1) is a and a._method == "std" and a._ddof == 1 and a._axis == (0,)
    assert a.sum() is a and a._method == "sum"
    a.method = "var"
    assert a.method is np.ma.var and a._ddof == 0
    a.method = "std"
    assert a.method is np.ma.std


def test_unknown_method_error_unchanged():
    a = Active(_var())
    with pytest.raises(ValueError, match="Choose from min/max/mean/sum"):
        a.method = "median"


@pytest.mark.parametrize("ddof", [-1, 1.5, True, "1"])
def test_bad_ddof(ddof):
    a = Active(_var())
    with pytest.raises(ValueError):
        a.var(ddof=ddof)
    with pytest.raises(ValueError):
        a.std(ddof=ddof)


def test_group_not_implemented_before_any_device_call(monkeypatch):
    from pyactivestorage_amd import active as mod

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(mod, "get_context", no_device)
    for method in ("var", "std"):
        a = Active(_var(), group=object())
        with pytest.raises(NotImplementedError, match="var/std with group="):
            getattr(a, method)()[...]
