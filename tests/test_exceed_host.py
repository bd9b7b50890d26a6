"""Host side of ``Active.exceed``: the record's layout, the exported C entry
points, ``exceed.check_field`` / ``finalize`` / ``merge`` on hand-made records,
and the ``Active`` API checks that run before any device call."""
import ctypes

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, exceed
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

ENTRY_POINTS = ("pyas_exceed_axes", "pyas_exceed_cols", "pyas_exceed_combine_segments", "pyas_exceed_combine_grid",
                "pyas_exceed_finalize")


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


# -- the record and the library -----------------------------------------------------------
def test_record_layout():
    assert ctypes.sizeof(_lib.Exceed) == 32 and _lib.EXCEED_NBYTES == 32
    assert [(f[0], getattr(_lib.Exceed, f[0]).offset) for f in _lib.Exceed._fields_] == \
        [("n", 0), ("n_true", 8), ("sum", 16), ("excess", 24)]
    dt = engine.exceed_dtype
    assert dt.itemsize == 32 == _lib.EXCEED_NBYTES and dt.names == ("n", "n_true", "sum", "excess") == exceed.FIELDS
    assert [dt.fields[name][1] for name in dt.names] == [0, 8, 16, 24]
    assert [dt.fields[name][0] for name in dt.names] == [np.dtype("<i8"), np.dtype("<i8"), np.dtype("<f8"),
                                                         np.dtype("<f8")]
    assert [(f[0], getattr(_lib.ExceedRule, f[0]).offset) for f in _lib.ExceedRule._fields_] == \
        [("op", 0), ("reserved", 4), ("threshold", 8), ("field", 16)]
    assert ctypes.sizeof(_lib.ExceedRule) == 24
    assert [(f[0], getattr(_lib.ExceedField, f[0]).offset) for f in _lib.ExceedField._fields_] == \
        [("values", 0), ("origin", 8), ("stride", 16)]
    assert ctypes.sizeof(_lib.ExceedField) == 16 + 8 * _lib.MAX_DIMS
    assert _lib.EXCEED_STATS == {"count": 0, "fraction": 1, "sum": 2, "mean": 3, "excess": 4}
    assert tuple(_lib.EXCEED_STATS) == exceed.STATS


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2 and _lib.ABI_VERSION == 2


def test_rule_struct_keeps_its_field():
    r = engine.exceed_rule("le", 2.5)
    assert (r.op, r.threshold, bool(r.field)) == (3, 2.5, False)
    r = engine.exceed_rule("gt", 0.0, (4096, 8192, [12, 4, 0]))
    f = r.field.contents
    assert (r.op, f.values, f.origin, list(f.stride)) == (0, 4096, 8192, [12, 4, 0] + [0] * (_lib.MAX_DIMS - 3))


# -- check_stat / check_field ---------------------------------------------------------------
def test_check_stat():
    for s in exceed.STATS:
        assert exceed.check_stat(s) == s
    for bad in ("longest", "COUNT", None, 0):
        with pytest.raises(ValueError, match="stat must be one of"):
            exceed.check_stat(bad)


def test_check_field_scalar():
    f = exceed.check_field(3, (4, 5), (0,))
    assert (f.scalar, f.values, f.mask, f.all_masked) == (3.0, None, None, False) and isinstance(f.scalar, float)
    assert exceed.check_field(np.float32(1.5), (4, 5), (0, 1)).scalar == 1.5
    for bad in (np.nan, np.inf, -np.inf, True, "3", None, 1j):
        with pytest.raises(ValueError, match="threshold must be a finite number"):
            exceed.check_field(bad, (4, 5), (0,))


def test_check_field_shapes():
    shape = (4, 5, 6)
    f = exceed.check_field(np.arange(30, dtype=np.int32).reshape(1, 5, 6), shape, (0,))
    assert f.scalar is None and f.values.dtype == np.float64 and f.values.shape == (1, 5, 6) and f.mask is None
    assert f.values.flags.c_contiguous and f.values[0, 2, 3] == 15.0
    assert exceed.check_field(np.zeros((4, 1, 6)), shape, (1,)).values.shape == (4, 1, 6)
    assert exceed.check_field(np.zeros((1, 1, 6)), shape, (0, 1)).values.shape == (1, 1, 6)
    assert exceed.check_field([[[1.0]] * 5], shape, (0, 2)).values.shape == (1, 5, 1)
    with pytest.raises(ValueError, match="must have 3 dimensions"):
        exceed.check_field(np.zeros((5, 6)), shape, (0,))
    with pytest.raises(ValueError, match="must have 3 dimensions"):
        exceed.check_field(np.zeros(6), shape, (0, 1))
    for bad in ((4, 5, 6), (1, 5, 5), (1, 1, 6), (1, 6, 5)):
        with pytest.raises(ValueError, match=r"must have shape \(1, 5, 6\)"):
            exceed.check_field(np.zeros(bad), shape, (0,))
    with pytest.raises(ValueError, match="not numeric"):
        exceed.check_field(np.array([[["a"] * 6] * 5]), shape, (0,))


def test_check_field_finite_and_masked():
    shape = (4, 5)
    for bad in (np.nan, np.inf, -np.inf):
        t = np.zeros((1, 5))
        t[0, 3] = bad
        with pytest.raises(ValueError, match="finite everywhere"):
            exceed.check_field(t, shape, (0,))
        with pytest.raises(ValueError, match="finite everywhere"):         # unmasked in a masked array too
            exceed.check_field(np.ma.MaskedArray(t, mask=[[1, 0, 0, 0, 0]]), shape, (0,))
        f = exceed.check_field(np.ma.MaskedArray(t, mask=[[0, 0, 0, 1, 0]]), shape, (0,))   # masked: accepted
        assert f.mask.tolist() == [[False, False, False, True, False]]
        assert np.isnan(f.values[0, 3]) and np.isfinite(np.delete(f.values[0], 3)).all()
    t = np.ma.MaskedArray(np.arange(5.0).reshape(1, 5), mask=False)
    f = exceed.check_field(t, shape, (0,))
    assert f.mask is None and f.values.tolist() == [[0.0, 1.0, 2.0, 3.0, 4.0]]
    t = np.arange(5.0).reshape(1, 5)
    f = exceed.check_field(t, shape, (0,))
    f.values[0, 0] = 9.0
    assert t[0, 0] == 0.0                                                   # a copy: the caller's array is untouched


def test_check_field_with_every_dim_reduced_is_the_scalar_case():
    f = exceed.check_field(np.full((1, 1), 2.5), (4, 5), (0, 1))
    assert (f.scalar, f.values, f.mask, f.all_masked) == (2.5, None, None, False)
    f = exceed.check_field(np.ma.MaskedArray([[2.5]], mask=[[True]]), (4, 5), (0, 1))
    assert f.values is None and f.all_masked and f.mask.tolist() == [[True]]
    with pytest.raises(ValueError, match=r"must have shape \(1, 1\)"):
        exceed.check_field(np.zeros((1, 5)), (4, 5), (0, 1))


# -- finalize / merge on hand-made records ----------------------------------------------------
#                      n  n_true  sum   excess
RECS = exceed.records([0, 4, 4, 1, 7], [0, 0, 3, 1, 2], [0.0, 0.0, 7.5, -2.0, np.inf], [0.0, 0.0, 1.5, 0.25, np.nan])


def test_finalize_every_stat_and_mask_rule():
    no_n, no_true = [True, False, False, False, False], [True, True, False, False, False]
    c = exceed.finalize(RECS, "count")
    assert c.dtype == np.int64 and c.mask.tolist() == no_n and c.data.tolist() == [0, 0, 3, 1, 2]
    f = exceed.finalize(RECS, "fraction")
    assert f.dtype == np.float64 and f.mask.tolist() == no_n and f.data.tolist() == [0.0, 0.0, 0.75, 1.0, 2 / 7]
    s = exceed.finalize(RECS, "sum")
    assert s.dtype == np.float64 and s.mask.tolist() == no_n and s.data.tolist() == [0.0, 0.0, 7.5, -2.0, np.inf]
    m = exceed.finalize(RECS, "mean")
    assert m.dtype == np.float64 and m.mask.tolist() == no_true and m.data.tolist() == [0.0, 0.0, 2.5, -2.0, np.inf]
    e = exceed.finalize(RECS, "excess")
    assert e.dtype == np.float64 and e.mask.tolist() == no_n
    assert e.data[:4].tolist() == [0.0, 0.0, 1.5, 0.25] and np.isnan(e.data[4])
    assert exceed.finalize(RECS).tolist() == c.tolist()                      # the default stat
    with pytest.raises(ValueError, match="stat must be one of"):
        exceed.finalize(RECS, "days")


def test_finalize_masks_where_the_threshold_is_masked():
    tm = np.array([False, False, True, False, True])
    for stat in exceed.STATS:
        plain, got = exceed.finalize(RECS, stat), exceed.finalize(RECS, stat, tm)
        assert got.mask.tolist() == (plain.mask | tm).tolist(), stat
        assert got.data[2] == 0 and got.data[4] == 0 and got.dtype == plain.dtype, stat
        assert got.data[3] == plain.data[3], stat
    grid = exceed.finalize(RECS.reshape(5, 1), "count", np.array([[True], [False], [False], [False], [False]]))
    assert grid.shape == (5, 1) and grid.mask[:, 0].tolist() == [True, False, False, False, False]


def test_finalize_reads_components():
    comps = {k: np.ma.MaskedArray(RECS[k].copy(), mask=False) for k in exceed.FIELDS}
    for stat in exceed.STATS:
        a, b = exceed.finalize(comps, stat), exceed.finalize(RECS, stat)
        assert a.mask.tolist() == b.mask.tolist() and a.data.tobytes() == b.data.tobytes(), stat


def test_merge_adds_field_by_field():
    a = exceed.records([3, 0, 5], [1, 0, 5], [2.5, 0.0, 1e300], [0.5, 0.0, 1.0])
    b = exceed.records([4, 0, 1], [0, 0, 1], [0.0, 0.0, 1e300], [0.0, 0.0, 2.0])
    m = exceed.merge(a, b)
    assert m.dtype == engine.exceed_dtype
    assert m["n"].tolist() == [7, 0, 6] and m["n_true"].tolist() == [1, 0, 6]
    assert m["sum"].tolist() == [2.5, 0.0, 2e300] and m["excess"].tolist() == [0.5, 0.0, 3.0]
    zero = np.zeros(3, dtype=engine.exceed_dtype)
    assert exceed.merge(a, zero).tobytes() == a.tobytes() == exceed.merge(zero, a).tobytes()   # the neutral record
    assert exceed.merge(b, a).tobytes() == m.tobytes()                                          # commutative
    one = exceed.merge(a, b[:1])                                                                # broadcast
    assert one["n"].tolist() == [7, 4, 9]
    comps = lambda r: {k: np.ma.MaskedArray(r[k].copy(), mask=False) for k in exceed.FIELDS}
    assert exceed.merge(comps(a), comps(b)).tobytes() == m.tobytes()


# -- Active's checks, before any device call -------------------------------------------------
def test_argument_checks(no_device):
    a = Active(_var())
    with pytest.raises(ValueError, match="exceed: op must be one of gt, ge, lt, le"):
        a.exceed("eq", 1.0)
    with pytest.raises(ValueError, match="exceed: stat must be one of count, fraction, sum, mean, excess"):
        a.exceed("gt", 1.0, "longest")
    for bad in (np.nan, np.inf, -np.inf, "1", True):
        with pytest.raises(ValueError, match="exceed: threshold must be a finite number"):
            a.exceed("gt", bad)
    with pytest.raises(ValueError, match="exceed: a threshold field must have 3 dimensions"):
        a.exceed("gt", np.zeros((3, 4)), axis=(0,))
    with pytest.raises(ValueError, match=r"exceed: a threshold field must have shape \(1, 3, 4\)"):
        a.exceed("gt", np.zeros((2, 3, 4)), axis=(0,))
    with pytest.raises(ValueError, match=r"exceed: a threshold field must have shape \(2, 1, 4\)"):
        a.exceed("gt", np.zeros((1, 3, 4)), axis=(1,))
    t = np.zeros((1, 3, 4))
    t[0, 1, 1] = np.nan
    with pytest.raises(ValueError, match="exceed: a threshold field must be finite everywhere"):
        a.exceed("gt", t, axis=(0,))
    with pytest.raises(ValueError, match="out-of-range axis"):
        a.exceed("gt", 1.0, axis=(3,))
    assert a._exceed is None and a._method is None                                # nothing was set by the failures


def test_settings_hold_for_one_query(no_device):
    a = Active(_var())
    t = np.ma.MaskedArray(np.zeros((1, 3, 4)), mask=False)
    t[0, 2, 3] = np.ma.masked
    assert a.exceed("le", t, "mean", axis=(0,)) is a                              # a masked field is accepted
    assert a._method == "exceed" and a._axis == (0,) and a.method is None
    ex = a._exceed
    assert (ex["op"], ex["stat"], ex["axes"]) == ("le", "mean", (0,)) and ex["field"].mask[0, 2, 3]
    a.method = "mean"                                                             # the method setter clears it
    assert a._exceed is None
    a.exceed("gt", 1.0)                                                           # the axis stays, as for var
    assert a._exceed["axes"] == (0,) and a._exceed["field"].scalar == 1.0
    a = Active(_var())
    a.exceed("gt", 1.0)
    assert a._exceed["axes"] == (0, 1, 2)
    with pytest.raises(IndexError):                                               # an index that drops an axis
        a[0]
    assert a._exceed is None and a._method is None                                # __getitem__ cleared it
    assert a.exceed_path is None
    b = Active(_var(), axis=1)                                                    # the constructor's axis
    b.exceed("gt", np.zeros((2, 1, 4)))
    assert b._exceed["axes"] == (1,)


def test_group_raises(no_device):
    a = Active(_var(), group=object())
    a.exceed("gt", 1.0, axis=(0,))
    with pytest.raises(NotImplementedError, match="exceed with group="):
        a[...]
    assert a._exceed is None


def test_empty_selection_needs_no_device(no_device):
    a = Active(_var())
    for stat in exceed.STATS:
        r = a.exceed("gt", 1.0, stat, axis=(0,))[:, 1:1]
        assert r.shape == (1, 0, 4) and r.dtype == (np.int64 if stat == "count" else np.float64)
        assert isinstance(r, np.ma.MaskedArray) and a.exceed_path is None
    r = a.exceed("gt", 1.0, "sum", axis=(0, 1, 2))[0:0]
    assert r.shape == (1, 1, 1) and r.mask.all() and r.dtype == np.float64
    a.components = True
    c = a.exceed("gt", np.zeros((1, 3, 4)), axis=(0,))[0:0]
    assert set(c) == set(exceed.FIELDS)
    assert c["n"].dtype == np.int64 and c["n_true"].dtype == np.int64 and c["sum"].dtype == np.float64
    assert all(v.shape == (1, 3, 4) and not np.ma.getmaskarray(v).any() and (v.data == 0).all() for v in c.values())
