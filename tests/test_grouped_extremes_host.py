"""Host side of ``Active.grouped("min" | "max" | "sum")``: the new bindings,
``grouped.finalize`` over hand-made ``engine.partial_dtype`` records,
``grouped.merge_partials`` and the settings of a query that reaches no
device."""
import ctypes

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, grouped
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable


def _var(dt="<f4", shape=(2, 3, 4)):
    data = np.arange(int(np.prod(shape))).astype(dt).reshape(shape)
    raw = data.tobytes()
    return ChunkedVariable(name="v", shape=data.shape, chunks=data.shape, dtype=np.dtype(dt),
                           chunk_index={(0,) * len(shape): (0, len(raw))}, reader=lambda off, size: raw[off:off + size])


def _recs(dt, rows):
    """``partial_dtype(dt)`` records from (sum, count, min, max) tuples."""
    return np.array(rows, dtype=engine.partial_dtype(dt))


def test_bindings_and_stats():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    with open(_lib.LIB_DIR + "/../../include/pyas.h") as f:
        header = f.read()
    for name in ("pyas_group_cols_partial", "pyas_group_axes_partial"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
        assert f"int {name}(pyas_ctx *ctx" in header, name
    assert len(_lib.SIGNATURES["pyas_group_cols_partial"]) == len(_lib.SIGNATURES["pyas_group_cols"])
    assert len(_lib.SIGNATURES["pyas_group_axes_partial"]) == len(_lib.SIGNATURES["pyas_group_axes"])
    assert grouped.STATS == ("mean", "var", "std", "count", "min", "max", "sum")
    assert _lib.PARTIAL_NBYTES == _lib.MOMENTS_NBYTES == 32      # the record cap counts 32 B for either record


def test_settings_are_stored_and_cleared(monkeypatch):
    from pyactivestorage_amd import active as mod
    monkeypatch.setattr(mod, "get_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    a = Active(_var())
    assert a.grouped("max", 0, [0, 1], axis=(0,), ddof=3) is a
    assert a._method == "grouped" and a._grouped["stat"] == "max" and a._grouped["n_groups"] == 2 and a._ddof == 3
    # no group, and no selected element: right-shaped, right-typed, all masked, no launch
    for stat, dt, want in (("max", "<f4", np.float32), ("min", ">i2", np.int16), ("sum", "<f4", np.float32),
                           ("sum", "<i2", np.int64), ("sum", "|u1", np.uint64), ("min", "<u8", np.uint64)):
        a = Active(_var(dt))
        got = a.grouped(stat, 0, [-1, -1], axis=(0,))[...]
        assert isinstance(got, np.ma.MaskedArray) and got.shape == (0, 3, 4) and got.dtype == want, (stat, dt)
        assert got.dtype.isnative and np.ma.getmaskarray(got).shape == got.shape
        got = a.grouped(stat, 0, [0, 1], axis=(0,), n_groups=3)[:, 1:1]
        assert got.shape == (3, 0, 4) and got.dtype == want and a.grouped_path is None
        assert a._grouped is None and a._method is None and a._ddof == 0
    a = Active(_var("<i2"))
    a.components = True
    comp = a.grouped("sum", 0, [-1, -1], axis=(0,), n_groups=0)[...]
    assert sorted(comp) == ["max", "min", "n", "sum"]
    assert comp["sum"].dtype == np.int64 and comp["min"].dtype == np.int16 and comp["n"].dtype == np.int64
    assert all(v.shape == (0, 3, 4) for v in comp.values())


def test_bad_arguments():
    for kw in (dict(stat="median", along=0, labels=[0, 1]),
               dict(stat="max", along=0, labels=[0, 1], ddof=-1),
               dict(stat="sum", along=0, labels=[0, 2], n_groups=2),
               dict(stat="min", along=3, labels=[0, 1])):
        with pytest.raises(ValueError):
            Active(_var()).grouped(**kw)


def test_query_time_errors(monkeypatch):
    from pyactivestorage_amd import active as mod
    monkeypatch.setattr(mod, "get_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="grouped with group="):
        a.grouped("max", 0, [0, 1], axis=(0,))[...]
    a = Active(_var())
    with pytest.raises(ValueError, match="not among the reduced axes"):
        a.grouped("sum", 0, [0, 1], axis=(1,))[...]
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.weights = {0: [1.0, 2.0]}
        a.grouped("sum", 0, [0, 1], axis=(0,))[...]
    assert a._weights is None and a._grouped is None
    monkeypatch.setattr(mod.histogram, "TABLE_CAP_BYTES", 12 * 2 * 32 - 1)
    with pytest.raises(ValueError, match="above the cap"):
        a.grouped("min", 0, [0, 1], axis=(0,))[...]


# -- finalize -------------------------------------------------------------------
def test_finalize_dtypes_masks_values():
    for dt in ("<f4", ">f4", "<f8", "<i2", "|u1", "<i8", "<u8"):
        _finalize_dtypes_masks_values(dt)


def _finalize_dtypes_masks_values(dt):
    d = np.dtype(dt)
    big = {"<i8": 2 ** 60 + 1, "<u8": 2 ** 63 + 5}.get(dt, 7)
    # three values, nothing counted (fields that mean nothing), one element
    parts = _recs(dt, [[(big + 3, 3, 1, big), (99, 0, 55, 44), (5, 1, 5, 5)]])
    nat = d.newbyteorder("=")
    for stat, want, vals in (("min", nat, [1, 0, 5]), ("max", nat, [big, 0, 5]),
                             ("sum", nat if d.kind == "f" else np.dtype("int64" if d.kind == "i" else "uint64"),
                              [big + 3, 0, 5])):
        got = grouped.finalize(parts, stat, dtype=d)
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == want and got.dtype.isnative and got.shape == (1, 3)
        assert np.ma.getmaskarray(got).tolist() == [[False, True, False]], stat
        assert np.array_equal(got.data, np.array([[np.dtype(want).type(v) for v in vals]])), (stat, got.data)
        assert grouped.finalize(parts, stat, ddof=3, dtype=d).tobytes() == got.tobytes()
    if d.kind in "iu" and d.itemsize == 8:      # beyond 2^53: nothing went through float64
        assert int(grouped.finalize(parts, "max", dtype=d).data[0, 0]) == big
        assert int(grouped.finalize(parts, "sum", dtype=d).data[0, 0]) == big + 3
    with pytest.raises(ValueError):
        grouped.finalize(parts, "median", dtype=d)
    with pytest.raises(ValueError):             # moments records are not partial records
        grouped.finalize(np.zeros(2, dtype=engine.moments_dtype), "max", dtype=d)


def test_finalize_nan_and_f32_rounding():
    parts = _recs("<f4", [(np.nan, 2, np.nan, np.nan), (1.0 + 2.0 ** -30, 4, -np.inf, np.inf), (0.0, 0, 0.0, 0.0)])
    for stat in ("min", "max", "sum"):
        got = grouped.finalize(parts, stat, dtype="<f4")
        assert got.dtype == np.float32 and np.isnan(got.data[0]) and not np.ma.getmaskarray(got)[0]
        assert np.ma.getmaskarray(got)[2]
    assert grouped.finalize(parts, "sum", dtype="<f4").data[1] == np.float32(1.0)      # the f64 sum rounded once
    assert grouped.finalize(parts, "sum", dtype="<f8").data[1] == 1.0 + 2.0 ** -30
    assert grouped.finalize(parts, "min", dtype="<f4").data[1] == -np.inf
    assert grouped.finalize(parts, "sum").dtype == np.float64                          # no dtype: the record's class


# -- merge_partials ---------------------------------------------------------------
def test_merge_partials_exact_cases():
    dt = "<i8"
    a = _recs(dt, [(10, 2, 3, 7), (0, 0, 123, -5), (2 ** 62, 1, 2 ** 62, 2 ** 62)])
    b = _recs(dt, [(-4, 1, -4, -4), (6, 2, 1, 5), (2 ** 62, 1, 2 ** 62, 2 ** 62)])
    c = _recs(dt, [(0, 0, 0, 0), (1, 1, 1, 1), (2 ** 62, 1, 2 ** 62, 2 ** 62)])
    ab = grouped.merge_partials(a, b)
    assert ab.dtype == a.dtype
    assert ab.tolist() == [(6, 3, -4, 7), (6, 2, 1, 5), (-2 ** 63, 2, 2 ** 62, 2 ** 62)]       # int64 wraps
    left = grouped.merge_partials(grouped.merge_partials(a, b), c)
    right = grouped.merge_partials(a, grouped.merge_partials(b, c))
    assert left.tobytes() == right.tobytes()                                                  # associative
    assert left.tolist()[2] == (-2 ** 62, 3, 2 ** 62, 2 ** 62)       # three 2^62 wrap to -2^62, as NumPy's sum does
    assert int(np.full(3, 2 ** 62, dtype=np.int64).sum()) == -2 ** 62
    # the empty side is neutral, whatever its other fields hold
    empty = _recs(dt, [(77, 0, -99, 99)] * 3)
    assert grouped.merge_partials(a, empty).tobytes() == a.tobytes()
    assert grouped.merge_partials(empty, a)[[0, 2]].tobytes() == a[[0, 2]].tobytes()
    assert grouped.merge_partials(empty, empty)["count"].tolist() == [0, 0, 0]
    u = grouped.merge_partials(_recs("<u8", [(2 ** 63, 1, 2 ** 63, 2 ** 63)]), _recs("<u8", [(2 ** 63 + 1, 1, 2 ** 63 + 1,
                                                                                             2 ** 63 + 1)]))
    assert u.tolist() == [(1, 2, 2 ** 63, 2 ** 63 + 1)]                                        # uint64 wraps, exact extremes


def test_merge_partials_floats():
    nan = np.nan
    a = _recs("<f4", [(3.0, 2, 1.0, 2.0), (nan, 1, nan, nan), (1.0, 1, 1.0, 1.0), (np.inf, 1, np.inf, np.inf)])
    b = _recs("<f4", [(0.5, 1, 0.5, 0.5), (1.0, 1, 1.0, 1.0), (nan, 1, nan, nan), (-np.inf, 1, -np.inf, -np.inf)])
    m = grouped.merge_partials(a, b)
    assert m[0].tolist() == (3.5, 3, 0.5, 2.0)
    for k in (1, 2):                                       # a NaN on either side gives NaN
        assert m["count"][k] == 2 and all(np.isnan(m[f][k]) for f in ("sum", "min", "max"))
    assert np.isnan(m["sum"][3]) and m["min"][3] == -np.inf and m["max"][3] == np.inf
    assert grouped.merge_partials(a[0], b).shape == (4,)   # broadcast
    with pytest.raises(ValueError):
        grouped.merge_partials(a, _recs("<i2", [(0, 0, 0, 0)] * 4))
    with pytest.raises(ValueError):
        grouped.merge_partials(np.zeros(1, dtype=engine.moments_dtype), np.zeros(1, dtype=engine.moments_dtype))
