"""Host side of ``Active.argmax`` / ``Active.argmin``: the record's layout, the
exported C entry points, ``argext.of`` / ``merge`` / ``finalize`` against a
per-output Python loop, and the ``Active`` API checks that run before any
device call."""
import ctypes
import itertools

import numpy as np
import pytest

from pyactivestorage_amd import _lib, argext, engine
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

ENTRY_POINTS = ("pyas_argext_axes", "pyas_argext_cols", "pyas_argext_combine_segments", "pyas_argext_combine_grid",
                "pyas_argext_finalize")
DTYPES = ("|i1", "|u1", "<i2", "<u2", "<i4", "<u4", "<i8", "<u8", "<f4", "<f8")


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
    assert ctypes.sizeof(_lib.Argext) == 16 and _lib.ARGEXT_NBYTES == 16
    assert [(f[0], getattr(_lib.Argext, f[0]).offset) for f in _lib.Argext._fields_] == \
        [("value", 0), ("index", 8), ("n", 12)]
    dt = engine.argext_dtype
    assert dt.itemsize == 16 and dt.names == ("value", "index", "n") == argext.FIELDS
    assert [dt.fields[name][1] for name in dt.names] == [0, 8, 12]
    assert [dt.fields[name][0] for name in dt.names] == [np.dtype("<u8"), np.dtype("<i4"), np.dtype("<i4")]
    assert [(f[0], getattr(_lib.ArgextRule, f[0]).offset) for f in _lib.ArgextRule._fields_] == \
        [("dim", 0), ("which", 4), ("origin", 8)]
    assert ctypes.sizeof(_lib.ArgextRule) == 16
    assert _lib.ARGEXT_WHICH == {"max": 0, "min": 1}


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2 and _lib.ABI_VERSION == 2


# -- of / merge / finalize against a loop ---------------------------------------------------
def brute(seq, ok, which):
    """(index, value, n) of one sequence by the rules, element by element:
    the first unmasked NaN, else the first unmasked element equal to the
    unmasked extreme."""
    live = [i for i in range(len(seq)) if ok[i]]
    if not live:
        return 0, None, 0
    nans = [i for i in live if seq[i] != seq[i]]
    if nans:
        return nans[0], seq[nans[0]], len(live)
    ext = (max if which == "max" else min)(seq[i] for i in live)
    first = [i for i in live if seq[i] == ext][0]
    return first, seq[first], len(live)


def sample(dt, shape, seed, nan=0.15):
    """Few distinct values, so ties abound; both zeros and NaNs for floats;
    neighbours near the top of the 8-byte types that tie as float64."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(dt)
    if dt.kind == "f":
        x = rng.choice(np.array([-2.0, -0.0, 0.0, 1.5, 3.0], dtype=dt), size=shape)
        x[rng.random(shape) < nan] = np.nan
        return x
    info = np.iinfo(dt)
    pool = np.array([info.min, info.min + 1, 0, 1, info.max - 1, info.max], dtype=dt)
    return rng.choice(pool, size=shape)


def check_against_brute(rec, x, ok, along, which):
    x2 = np.moveaxis(x, along, 0).reshape(x.shape[along], -1)
    o2 = np.moveaxis(ok, along, 0).reshape(x.shape[along], -1)
    flat = rec.reshape(-1)
    vals = argext.values(rec, x.dtype).reshape(-1)
    for c in range(x2.shape[1]):
        i, v, n = brute(x2[:, c], o2[:, c], which)
        assert flat["n"][c] == n, (c, which)
        if n == 0:
            assert flat[c].tobytes() == bytes(16), c          # the neutral record is all zero
            continue
        assert flat["index"][c] == i, (c, which, x2[:, c], o2[:, c])
        assert vals[c].tobytes() == np.asarray(v, dtype=x.dtype.newbyteorder("=")).tobytes(), (c, which)


@pytest.mark.parametrize("dt", DTYPES + (">f4", ">i8"))
def test_of_against_a_loop(dt):
    x = sample(dt, (9, 5, 7), 11)
    ok = np.random.default_rng(12).random(x.shape) < 0.7
    ok[:, 0, 0] = False                                    # a wholly masked sequence
    for which in argext.WHICH:
        for along in (0, 1, -1):
            rec = argext.of(x, ok, along, which)
            assert rec.dtype == engine.argext_dtype and rec.shape == tuple(np.delete(x.shape, along))
            check_against_brute(rec, x, ok, along, which)
        check_against_brute(argext.of(x, None, 0, which), x, np.ones(x.shape, bool), 0, which)


def test_of_compares_in_the_variables_type():
    """Neighbours that tie after astype(float64) do not tie."""
    x = np.array([2 ** 60, 2 ** 60 + 1, 2 ** 60 + 1, 2 ** 60 - 1, 2 ** 60 - 1], dtype="<i8")
    assert float(x[0]) == float(x[1]) == float(x[3])
    assert argext.of(x, None, 0, "max")["index"] == 1 and argext.of(x, None, 0, "min")["index"] == 3
    u = np.array([2 ** 63, 2 ** 63 + 1, 2 ** 63 + 1, 2 ** 63 - 1, 2 ** 63 - 1], dtype="<u8")
    assert float(u[0]) == float(u[1]) == float(u[3])
    r = argext.of(u, None, 0, "max")
    assert r["index"] == 1 and argext.values(r, u.dtype) == u[1]
    r = argext.of(u, None, 0, "min")
    assert r["index"] == 3 and argext.values(r, u.dtype) == u[3]


def test_zero_signs_and_nans():
    x = np.array([-0.0, 0.0, -0.0], dtype="<f4")
    for which in argext.WHICH:
        r = argext.of(x, None, 0, which)
        assert r["index"] == 0 and np.signbit(argext.values(r, x.dtype))      # the first zero, its own sign
        r = argext.of(x[1:], None, 0, which)
        assert r["index"] == 0 and not np.signbit(argext.values(r, x.dtype))
    y = np.array([5.0, np.nan, 9.0, np.nan], dtype="<f8")
    for which in argext.WHICH:
        assert argext.of(y, None, 0, which)["index"] == 1                      # the first NaN, argmin too
        assert argext.of(y, [True, False, True, True], 0, which)["index"] == 3  # a masked NaN does not count


def _random_records(dt, n, seed):
    """Records with few values and few indices (ties in both), ``n == 0``
    records and NaN records among them."""
    rng = np.random.default_rng(seed)
    x = sample(dt, n, seed + 1, nan=0.3)
    cnt = rng.integers(0, 3, n)
    return argext.records(x, rng.integers(0, 4, n), cnt, dt)


@pytest.mark.parametrize("dt", DTYPES)
def test_merge_is_associative_and_commutative(dt):
    n = 4000
    a, b, c = (_random_records(dt, n, s) for s in (1, 5, 9))
    zero = np.zeros(n, dtype=engine.argext_dtype)
    for which in argext.WHICH:
        m = lambda p, q: argext.merge(p, q, which=which, dtype=dt)
        assert m(a, b).tobytes() == m(b, a).tobytes()
        assert m(m(a, b), c).tobytes() == m(a, m(b, c)).tobytes() == m(m(c, a), b).tobytes()
        assert m(a, zero).tobytes() == a.tobytes() == m(zero, a).tobytes()      # n == 0 is neutral
        assert m(zero, zero).tobytes() == zero.tobytes()
        assert (m(a, b)["n"] == a["n"] + b["n"]).all()


@pytest.mark.parametrize("dt", ["<f4", "<f8", "<i1", "<i8", "<u8", "<u2"])
def test_merge_with_shift_equals_of_on_the_concatenation(dt):
    x = sample(dt, (12, 40), 21)
    ok = np.random.default_rng(22).random(x.shape) < 0.6
    for which in argext.WHICH:
        whole = argext.of(x, ok, 0, which)
        for cut in (0, 1, 5, 11, 12):
            a, b = argext.of(x[:cut], ok[:cut], 0, which), argext.of(x[cut:], ok[cut:], 0, which)
            assert argext.merge(a, b, cut, which=which, dtype=dt).tobytes() == whole.tobytes(), (which, cut)
            assert argext.merge(a, b, shift=cut, which=which, dtype=dt).tobytes() == whole.tobytes()
        # three parts, both association orders
        a, b, c = (argext.of(x[lo:hi], ok[lo:hi], 0, which) for lo, hi in ((0, 4), (4, 9), (9, 12)))
        m = lambda p, q, s: argext.merge(p, q, s, which=which, dtype=dt)
        assert m(m(a, b, 4), c, 9).tobytes() == m(a, m(b, c, 5), 4).tobytes() == whole.tobytes()


def test_merge_reads_components_dicts():
    x = sample("<f4", (8, 6), 31)
    rec = [argext.of(x[lo:hi], None, 0, "max") for lo, hi in ((0, 3), (3, 8))]
    comp = [{"value": np.ma.MaskedArray(argext.values(r, x.dtype), mask=r["n"] == 0),
             "index": argext.finalize(r), "n": np.ma.MaskedArray(r["n"].astype(np.int64)),
             "position": argext.finalize(r)} for r in rec]
    want = argext.merge(rec[0], rec[1], 3, which="max", dtype=x.dtype)
    assert argext.merge(comp[0], comp[1], 3, which="max").tobytes() == want.tobytes()
    assert want.tobytes() == argext.of(x, None, 0, "max").tobytes()
    assert argext.finalize(comp[0]).tobytes() == argext.finalize(rec[0]).tobytes()
    with pytest.raises(ValueError, match="dtype"):
        argext.merge(rec[0], rec[1], 3, which="max")
    with pytest.raises(ValueError, match="which"):
        argext.merge(rec[0], rec[1], 3, which="mean", dtype=x.dtype)
    with pytest.raises(TypeError):
        argext.merge(rec[0], rec[1], 3, dtype=x.dtype)


def test_finalize_masks_empty_outputs():
    rec = argext.records(np.array([3.0, 1.0, 7.0]), [4, 9, 2], [2, 0, 1], "<f8")
    got = argext.finalize(rec)
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.int64
    assert np.ma.getmaskarray(got).tolist() == [False, True, False] and got.filled(-1).tolist() == [4, -1, 2]
    assert rec[1].tobytes() == bytes(16)
    assert np.ma.getmaskarray(argext.finalize(np.zeros((2, 3), dtype=engine.argext_dtype))).all()
    with pytest.raises(ValueError):
        argext.of(np.zeros((2, 2)), np.ones((3, 2), bool), 0, "max")
    with pytest.raises(ValueError):
        argext.of(np.zeros((2, 2)), None, 2, "max")
    with pytest.raises(ValueError):
        argext.of(np.zeros((2, 2)), None, 0, "mean")
    with pytest.raises(ValueError):
        argext.of(np.zeros((2, 2), dtype=complex), None, 0, "max")


# -- the Active API: every error before any device call --------------------------------
def test_api_returns_self_and_settings():
    a = Active(_var())
    assert a.argext_path is None
    assert a.argmax(0) is a and a._method == "argmax" and a._axis == (0,)
    assert a._argext["along"] == 0 and a._argext["which"] == "max"
    assert a.method is None               # not one of the reference's methods
    assert a.argmin(-1) is a and a._method == "argmin" and a._axis == (2,)
    assert a._argext["along"] == 2 and a._argext["which"] == "min"
    assert a.argmax(np.int64(1)) is a and a._axis == (1,)
    a.method = "mean"
    assert a._argext is None and a._method == "mean"
    a.argmin(1)
    a.method = None
    assert a._argext is None and a._method is None
    with pytest.raises(AttributeError):
        a.argext_path = "cols"


@pytest.mark.parametrize("name", ["argmax", "argmin"])
@pytest.mark.parametrize("along", [3, -4, True, 1.0, "0", None])
def test_bad_along(no_device, name, along):
    a = Active(_var())
    with pytest.raises(ValueError, match=f"{name}: along"):
        getattr(a, name)(along)
    assert a._method is None and a._argext is None


@pytest.mark.parametrize("name", ["argmax", "argmin"])
@pytest.mark.parametrize("index", [([1, 0],), ([0, 0, 1],), ([1, -2],), (np.array([1, 1]),),
                                   (slice(None, None, -1),), (1,)],
                         ids=["unsorted", "repeated", "negative-unsorted", "array-repeated", "negative-step", "int"])
def test_selection_along_must_keep_the_order(no_device, name, index):
    a = Active(_var())
    with pytest.raises(ValueError, match=f"{name}: the .* along dimension 0"):
        getattr(a, name)(0)[index]
    assert a._method is None and a._argext is None             # cleared after the failed query


def test_spell_messages_are_unchanged(no_device):
    """The order check is shared with spell: its words stay."""
    a = Active(_var())
    with pytest.raises(ValueError, match="^spell: the slice along dimension 0 has step -1; runs follow the "
                                         "selection in increasing order, so the step must be >= 1$"):
        a.spell(0, "gt", 0.0)[::-1]
    with pytest.raises(ValueError, match="^spell: the index list along dimension 0 must be strictly increasing "
                                         "\\(no repeats\\): runs follow the selection in order$"):
        a.spell(0, "gt", 0.0)[[1, 0]]
    with pytest.raises(ValueError, match="^spell: the index along dimension 0 must be a slice, an increasing index "
                                         "list or a boolean mask. Got 1$"):
        a.spell(0, "gt", 0.0)[1]


def test_kept_dims_take_any_list(no_device):
    """An unsorted list on a kept dim passes the order check (the query then
    goes on to the device: here, to the patched context)."""
    a = Active(_var())
    with pytest.raises(AssertionError, match="a device call was made"):
        a.argmax(0)[:, [2, 0], :]
    assert a._method is None and a._argext is None


def test_weights_are_refused(no_device):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.argmax(0)[...]
    assert a._argext is None and a._weights is None and a._method is None


@pytest.mark.parametrize("name", ["argmax", "argmin"])
def test_group_not_implemented(no_device, name):
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match=f"{name} with group="):
        getattr(a, name)(0)[...]
    assert a._argext is None and a._method is None


def test_too_long_a_selection(no_device):
    """2^31 positions along ``along``: refused before any device call (the
    variable is virtual)."""
    n = 2 ** 31
    var = ChunkedVariable(name="v", shape=(n, 2), chunks=(2 ** 20, 2), dtype=np.dtype("|i1"), chunk_index={},
                          reader=lambda off, size: b"")
    a = Active(var)
    with pytest.raises(NotImplementedError, match="2\\^31"):
        a.argmax(0)[...]
    assert a._argext is None and a._method is None
    # fewer positions, but indices past int32
    with pytest.raises(NotImplementedError, match="2\\^31"):
        Active(var).argmin(0)[::2]


def test_selection_position():
    """Global indices back to positions in the selection: a slice with a
    step, an index list, a boolean mask."""
    from pyactivestorage_amd.active import _selection_position
    from pyactivestorage_amd.indexing import OrthogonalIndexer
    none = np.zeros(3, dtype=bool)
    dims = OrthogonalIndexer((slice(3, 20, 4), [1, 4, 5, 9], np.arange(10) % 3 == 1), (23, 10, 10), (5, 5, 5)).dim_indexers
    assert _selection_position(np.array([3, 11, 19]), none, dims[0]).tolist() == [0, 2, 4]
    assert _selection_position(np.array([1, 5, 9]), none, dims[1]).tolist() == [0, 2, 3]
    assert _selection_position(np.array([1, 4, 7]), none, dims[2]).tolist() == [0, 1, 2]
    assert _selection_position(np.array([0, 11, 0]), np.array([True, False, True]), dims[0]).tolist() == [0, 2, 0]
    assert list(itertools.chain(range(3, 20, 4)))[2] == 11
