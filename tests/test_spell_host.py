"""Host side of ``Active.spell``: the record's layout, the exported C entry
points, ``spell.of`` / ``merge`` / ``finalize`` against a brute-force run-length
count, and the ``Active`` API checks that run before any device call."""
import ctypes
import itertools

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, spell
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

FIELDS = ("n", "n_true", "len", "head", "tail", "best", "days", "events", "min_length", "reserved")
ENTRY_POINTS = ("pyas_spell_axes", "pyas_spell_cols", "pyas_spell_combine_segments", "pyas_spell_combine_grid",
                "pyas_spell_finalize")


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
    assert ctypes.sizeof(_lib.Spell) == 40 and _lib.SPELL_NBYTES == 40
    assert [(f[0], getattr(_lib.Spell, f[0]).offset) for f in _lib.Spell._fields_] == \
        [(name, 4 * k) for k, name in enumerate(FIELDS)]
    assert engine.spell_dtype.itemsize == 40 and engine.spell_dtype.names == FIELDS
    assert [engine.spell_dtype.fields[name][1] for name in FIELDS] == [4 * k for k in range(10)]
    assert all(engine.spell_dtype.fields[name][0] == np.dtype("<i4") for name in FIELDS)
    assert ctypes.sizeof(_lib.SpellRule) == 24
    assert [(f[0], getattr(_lib.SpellRule, f[0]).offset) for f in _lib.SpellRule._fields_] == \
        [("dim", 0), ("op", 4), ("min_length", 8), ("threshold", 16)]
    assert _lib.SPELL_OPS == {"gt": 0, "ge": 1, "lt": 2, "le": 3}
    assert _lib.SPELL_STATS == {"longest": 0, "days": 1, "events": 2}


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2 and _lib.ABI_VERSION == 2


# -- merge and finalize against brute force ---------------------------------------------
def brute(seq, L):
    """(longest, days, events) of one boolean sequence by a run-length count."""
    runs, c = [], 0
    for b in seq:
        if b:
            c += 1
        else:
            if c:
                runs.append(c)
            c = 0
    if c:
        runs.append(c)
    return max(runs, default=0), sum(r for r in runs if r >= L), sum(1 for r in runs if r >= L)


def _stats(rec):
    return np.stack([np.ma.getdata(spell.finalize(rec, s)) for s in spell.STATS], axis=-1)


@pytest.mark.parametrize("L", [1, 2, 3, 6])
def test_merge_is_exact_and_associative(L):
    """Every boolean sequence up to length 8, every three-way split (empty
    parts included), both association orders."""
    for n in range(0, 9):
        seqs = np.array(list(itertools.product([False, True], repeat=n)), dtype=bool).reshape(2 ** n, n)
        want = np.array([brute(s, L) for s in seqs])
        whole = spell.of(seqs, None, 1, L)
        assert np.array_equal(_stats(whole), want), (n, L)
        for i in range(n + 1):
            for j in range(i, n + 1):
                a, b, c = (spell.of(seqs[:, lo:hi], None, 1, L) for lo, hi in ((0, i), (i, j), (j, n)))
                left = spell.merge(spell.merge(a, b), c)
                right = spell.merge(a, spell.merge(b, c))
                assert left.tobytes() == right.tobytes() == whole.tobytes(), (n, L, i, j)


def test_zero_record_is_neutral():
    rng = np.random.default_rng(3)
    seqs = rng.random((200, 17)) < 0.6
    valid = rng.random((200, 17)) < 0.9
    for L in (1, 3, 6):
        rec = spell.of(seqs, valid, 1, L)
        zero = np.zeros(rec.shape, dtype=engine.spell_dtype)
        assert spell.merge(zero, rec).tobytes() == rec.tobytes()
        assert spell.merge(rec, zero).tobytes() == rec.tobytes()
    assert spell.merge(zero, zero).tobytes() == zero.tobytes()
    assert np.ma.getmaskarray(spell.finalize(zero)).all()


def test_of_counts_and_masks():
    t = np.array([[1, 1, 0, 1, 1, 1, 0, 0, 1], [0, 0, 0, 0, 0, 0, 0, 0, 0], [1, 1, 1, 1, 1, 1, 1, 1, 1]], dtype=bool)
    v = np.ones_like(t)
    v[0, 4] = False                       # a masked position is false: it breaks the run of three
    v[1] = False                          # no unmasked position: masked
    rec = spell.of(t, v, -1, 2)
    assert rec.dtype == engine.spell_dtype and rec.shape == (3,)
    assert rec["n"].tolist() == [8, 0, 9] and rec["n_true"].tolist() == [5, 0, 9] and rec["len"].tolist() == [9] * 3
    assert rec["head"].tolist() == [2, 0, 9] and rec["tail"].tolist() == [1, 0, 9] and rec["best"].tolist() == [2, 0, 9]
    assert rec["days"].tolist() == [0, 0, 0] and rec["events"].tolist() == [0, 0, 0]     # the interior runs have length 1 < L
    for stat, want in (("longest", [2, 0, 9]), ("days", [2, 0, 9]), ("events", [1, 0, 1])):
        got = spell.finalize(rec, stat)
        assert got.dtype == np.int64 and np.ma.getmaskarray(got).tolist() == [False, True, False]
        assert got.filled(0).tolist() == want, stat
    # the components dict of a query is read like the records
    comp = {k: np.ma.MaskedArray(rec[k].astype(np.int64)) for k in spell.FIELDS}
    assert spell.finalize(comp, "days").tobytes() == spell.finalize(rec, "days").tobytes()
    assert spell.merge(comp, comp).tobytes() == spell.merge(rec, rec).tobytes()
    with pytest.raises(ValueError):
        spell.of(t, v[:2], 0)
    with pytest.raises(ValueError):
        spell.of(t, v, 2)
    with pytest.raises(ValueError):
        spell.finalize(rec, "mean")


# -- the Active API: every error before any device call --------------------------------
def test_api_returns_self_and_settings():
    a = Active(_var())
    assert a.spell_path is None
    assert a.spell(0, "gt", 1.5) is a and a._method == "spell" and a._axis == (0,)
    assert a._spell == {"along": 0, "op": "gt", "threshold": 1.5, "stat": "longest", "min_length": 1}
    assert a.method is None               # not one of the reference's methods
    assert a.spell(-1, "le", np.float32(2), stat="days", min_length=np.int64(6)) is a
    assert a._spell == {"along": 2, "op": "le", "threshold": 2.0, "stat": "days", "min_length": 6}
    assert a._axis == (2,)
    a.method = "mean"
    assert a._spell is None and a._method == "mean"
    a.spell(1, "lt", 0)
    a.method = None
    assert a._spell is None and a._method is None
    with pytest.raises(AttributeError):
        a.spell_path = "cols"


@pytest.mark.parametrize("along", [3, -4, True, 1.0, "0", None])
def test_bad_along(no_device, along):
    a = Active(_var())
    with pytest.raises(ValueError, match="along"):
        a.spell(along, "gt", 0.0)
    assert a._method is None and a._spell is None


@pytest.mark.parametrize("kw, word", [
    (dict(op="eq"), "op"), (dict(op=">"), "op"), (dict(op=None), "op"),
    (dict(threshold=np.nan), "threshold"), (dict(threshold=np.inf), "threshold"),
    (dict(threshold=-np.inf), "threshold"), (dict(threshold="1"), "threshold"), (dict(threshold=None), "threshold"),
    (dict(threshold=[1.0]), "threshold"), (dict(threshold=True), "threshold"),
    (dict(min_length=0), "min_length"), (dict(min_length=-1), "min_length"), (dict(min_length=2.0), "min_length"),
    (dict(min_length=True), "min_length"), (dict(min_length=None), "min_length"),
    (dict(stat="mean"), "stat"), (dict(stat=None), "stat"), (dict(stat="LONGEST"), "stat")])
def test_bad_settings(no_device, kw, word):
    a = Active(_var())
    args = dict(op="gt", threshold=0.0)
    args.update(kw)
    with pytest.raises(ValueError, match=word):
        a.spell(0, **args)
    assert a._method is None and a._spell is None


@pytest.mark.parametrize("index", [([1, 0],), ([0, 0, 1],), ([1, -2],), (np.array([1, 1]),),
                                   (slice(None, None, -1),), (1,)],
                         ids=["unsorted", "repeated", "negative-unsorted", "array-repeated", "negative-step", "int"])
def test_selection_along_must_keep_the_order(no_device, index):
    a = Active(_var())
    with pytest.raises(ValueError, match="spell: the .* along dimension 0"):
        a.spell(0, "gt", 0.0)[index]
    assert a._method is None and a._spell is None              # cleared after the failed query


def test_kept_dims_take_any_list(no_device):
    """An unsorted list on a kept dim passes the spell's own check (the
    query then goes on to the device: here, to the patched context)."""
    a = Active(_var())
    with pytest.raises(AssertionError, match="a device call was made"):
        a.spell(0, "gt", 0.0)[:, [2, 0], :]
    assert a._method is None and a._spell is None


def test_weights_are_refused(no_device):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.spell(0, "gt", 0.0)[...]
    assert a._spell is None and a._weights is None and a._method is None


def test_group_not_implemented(no_device):
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="spell with group="):
        a.spell(0, "gt", 0.0)[...]
    assert a._spell is None and a._method is None


def test_too_long_a_selection(no_device):
    """2^31 selected positions along ``along``: refused before any device call
    (a boolean mask of that length is never built: the variable is virtual)."""
    n = 2 ** 31
    var = ChunkedVariable(name="v", shape=(n, 2), chunks=(2 ** 20, 2), dtype=np.dtype("|i1"), chunk_index={},
                          reader=lambda off, size: b"")
    a = Active(var)
    with pytest.raises(NotImplementedError, match="2\\^31"):
        a.spell(0, "gt", 0.0)[...]
    assert a._spell is None and a._method is None
