"""Host side of ``Active.rolling``: the record's layout against the header, the
exported C entry points, ``rolling.of`` / ``merge`` / ``finalize`` against a
brute-force window scan written here, and the ``Active`` API checks that run
before any device call."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, rolling
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pyas.h")
FIELDS = ("best", "position", "n_windows", "n", "len", "window", "which", "head_ok", "tail_ok", "reserved", "head",
          "tail")
OFFSETS = (0, 8, 12, 16, 20, 24, 25, 26, 27, 28, 32, 88)
ENTRY_POINTS = ("pyas_roll_axes", "pyas_roll_cols", "pyas_roll_combine_segments", "pyas_roll_combine_grid",
                "pyas_roll_finalize")
WINDOWS = (1, 2, 3, 5, 8)


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
def test_record_layout_agrees_with_the_header():
    text = open(HEADER).read()
    cap = int(re.search(r"#define\s+PYAS_ROLL_MAX_WINDOW\s+(\d+)", text).group(1))
    assert cap == 8 == rolling.MAX_WINDOW == _lib.ROLL_MAX_WINDOW
    body = re.search(r"typedef struct \{([^}]*)\} pyas_roll;", text).group(1)
    names = [n.split("[")[0] for decl in body.split(";") if decl.strip()
             for n in re.sub(r"^\s*\w+\s+", "", decl.strip()).replace(" ", "").split(",")]
    assert tuple(names) == FIELDS
    assert "head[PYAS_ROLL_MAX_WINDOW - 1]" in body and "tail[PYAS_ROLL_MAX_WINDOW - 1]" in body
    assert ctypes.sizeof(_lib.Roll) == 144 and _lib.ROLL_NBYTES == 144
    assert [(f[0], getattr(_lib.Roll, f[0]).offset) for f in _lib.Roll._fields_] == list(zip(FIELDS, OFFSETS))
    assert engine.roll_dtype.itemsize == 144 and engine.roll_dtype.names == FIELDS
    assert tuple(engine.roll_dtype.fields[name][1] for name in FIELDS) == OFFSETS
    assert engine.roll_dtype["head"].shape == (7,) and engine.roll_dtype["tail"].shape == (7,)
    assert engine.roll_dtype["best"] == np.dtype("<f8") and engine.roll_dtype["position"] == np.dtype("<i4")
    assert set(rolling.FIELDS) == set(FIELDS) - {"reserved"}
    assert ctypes.sizeof(_lib.RollRule) == 12
    assert [(f[0], getattr(_lib.RollRule, f[0]).offset) for f in _lib.RollRule._fields_] == \
        [("dim", 0), ("window", 4), ("which", 8)]
    assert _lib.ROLL_WHICH == {"max": 0, "min": 1} and _lib.ROLL_STATS == {"sum": 0, "mean": 1}
    assert re.search(r"PYAS_ROLL_MAX = 0, PYAS_ROLL_MIN = 1", text) and re.search(r"PYAS_ROLL_SUM = 0, PYAS_ROLL_MEAN = 1", text)


def test_library_exports_entry_points():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert lib.pyas_abi_version() == 2 and _lib.ABI_VERSION == 2


# -- of, merge and finalize against brute force -------------------------------------------
def brute(x, ok, w, mn):
    """(sum, position, n_windows) of one sequence by a scan over the window
    starts; sum is None when no window is valid."""
    best, pos, nw = None, None, 0
    for p in range(len(x) - w + 1):
        if not all(ok[p:p + w]):
            continue
        s = np.float64(x[p])
        for j in range(1, w):
            s = s + np.float64(x[p + j])
        nw += 1
        if best is None:
            take = True
        elif best != best:
            take = False
        elif s != s:
            take = True
        else:
            take = s < best if mn else s > best
        if take:
            best, pos = s, p
    return best, pos, nw


def sequences(length):
    """(values, valid) of sequences of ``length`` over two small integers.

    Up to length 6 the full product: every value sequence under every validity
    pattern.  For lengths 7 and 8 the full product (4^8 sequences, each through
    45 splits, two association orders, five windows and two extremes) would
    take minutes on the host, so the two factors are crossed one at a time:
    every validity pattern under 8 value sequences, and every value sequence
    under 4 validity patterns, the all-valid one among them.  That suffices
    because the two enter the rule independently: which windows exist, which
    head and tail slots are set and how the counts add depends on the validity
    pattern alone (covered in full), and among the windows that exist the sums,
    the ties and which one wins depend on the values alone (covered in full
    where every window exists, which is where the most windows compete and
    where a window of 8 exists at all).  One small integer of either sign
    makes ties common and keeps every sum exact; ``test_nan_and_infinities``,
    ``test_ties_keep_the_first`` and the random ``test_zero_record_is_neutral``
    bring other values."""
    vals = [np.array(v, dtype=np.int64) for v in itertools.product((-1, 2), repeat=length)]
    oks = [np.array(o, dtype=bool) for o in itertools.product((True, False), repeat=length)]
    if length <= 6:
        pairs = list(itertools.product(vals, oks))
    else:
        rng = np.random.default_rng(length)
        few_v = [vals[k] for k in rng.choice(len(vals), 8, replace=False)]
        few_o = [oks[0]] + [oks[k] for k in rng.choice(np.arange(1, len(oks)), 3, replace=False)]
        pairs = list(itertools.product(few_v, oks)) + list(itertools.product(vals, few_o))
    x = np.array([p[0] for p in pairs]).reshape(len(pairs), length)
    ok = np.array([p[1] for p in pairs]).reshape(len(pairs), length)
    return x, ok


def same_records(a, b, what):
    for name in rolling.FIELDS:
        assert np.array_equal(a[name], b[name], equal_nan=name == "best"), (what, name)


@pytest.mark.parametrize("which", ["max", "min"])
@pytest.mark.parametrize("w", WINDOWS)
def test_of_merge_finalize_against_brute_force(w, which):
    mn = which == "min"
    for length in range(9):
        x, ok = sequences(length)
        whole = rolling.of(x, ok, 1, w, which)
        assert whole.shape == (len(x),) and (whole["len"] == length).all() and (whole["window"] == w).all()
        assert (whole["n"] == ok.sum(axis=1)).all() and (whole["which"] == int(mn)).all()
        value, mean = rolling.finalize(whole, "sum"), rolling.finalize(whole, "mean")
        for k in range(len(x)):
            best, pos, nw = brute(x[k], ok[k], w, mn)
            assert whole["n_windows"][k] == nw
            assert bool(np.ma.getmaskarray(value)[k]) == (best is None) == bool(np.ma.getmaskarray(mean)[k])
            if best is not None:
                assert value.data[k] == best and whole["position"][k] == pos and mean.data[k] == best / np.float64(w)
            c = min(length, w - 1)
            assert whole["head"][k].tolist() == [float(v) if o else 0.0 for v, o in zip(x[k][:c], ok[k][:c])] \
                + [0.0] * (7 - c)
            assert whole["tail"][k].tolist() == [float(v) if o else 0.0 for v, o in
                                                 zip(x[k][::-1][:c], ok[k][::-1][:c])] + [0.0] * (7 - c)
            assert whole["head_ok"][k] == sum(int(o) << j for j, o in enumerate(ok[k][:c]))
            assert whole["tail_ok"][k] == sum(int(o) << j for j, o in enumerate(ok[k][::-1][:c]))
        # every split into three pieces, empty ones included, in both association orders
        piece = {(i, j): rolling.of(x[:, i:j], ok[:, i:j], 1, w, which)
                 for i in range(length + 1) for j in range(i, length + 1)}
        for i in range(length + 1):
            for j in range(i, length + 1):
                a, b, c = piece[0, i], piece[i, j], piece[j, length]
                same_records(rolling.merge(rolling.merge(a, b), c), whole, (length, i, j, "left"))
                same_records(rolling.merge(a, rolling.merge(b, c)), whole, (length, i, j, "right"))


@pytest.mark.parametrize("which", ["max", "min"])
def test_long_seams_against_brute_force(which):
    """Sequences of 18 positions, longer than two windows of 8: every two-way
    split and every third three-way split, so that a seam has full tails and
    heads on both sides, 7 windows across it, and pieces shorter than w - 1
    between two long ones."""
    rng = np.random.default_rng(17)
    n = 18
    x, ok = rng.integers(-3, 4, (120, n)), rng.random((120, n)) < 0.85
    ok[:30] = True
    for w in WINDOWS:
        whole = rolling.of(x, ok, 1, w, which)
        value = rolling.finalize(whole)
        for k in range(len(x)):
            best, pos, nw = brute(x[k], ok[k], w, which == "min")
            assert whole["n_windows"][k] == nw and bool(np.ma.getmaskarray(value)[k]) == (best is None)
            if best is not None:
                assert value.data[k] == best and whole["position"][k] == pos
        for i in range(n + 1):
            a = rolling.of(x[:, :i], ok[:, :i], 1, w, which)
            same_records(rolling.merge(a, rolling.of(x[:, i:], ok[:, i:], 1, w, which)), whole, (w, i))
            for j in range(i, n + 1, 3):
                b, c = rolling.of(x[:, i:j], ok[:, i:j], 1, w, which), rolling.of(x[:, j:], ok[:, j:], 1, w, which)
                same_records(rolling.merge(rolling.merge(a, b), c), whole, (w, i, j, "left"))
                same_records(rolling.merge(a, rolling.merge(b, c)), whole, (w, i, j, "right"))


def test_zero_record_is_neutral():
    rng = np.random.default_rng(3)
    x, ok = rng.integers(-4, 5, (50, 12)), rng.random((50, 12)) < 0.8
    zero = np.zeros((), dtype=engine.roll_dtype)
    for w in WINDOWS:
        for which in ("max", "min"):
            r = rolling.of(x, ok, -1, w, which)
            same_records(rolling.merge(zero, r), r, "zero first")
            same_records(rolling.merge(r, zero), r, "zero last")
    assert np.ma.getmaskarray(rolling.finalize(zero)).all()


def test_ties_keep_the_first():
    x = np.array([1, 2, 2, 1, 2, 2, 1, -0.0, 0.0])
    r = rolling.of(x, None, 0, 2, "max")
    assert (r["best"], r["position"], r["n_windows"]) == (4.0, 1, 8)
    r = rolling.of(x, None, 0, 2, "min")
    assert (r["best"], r["position"]) == (0.0, 7)             # -0.0 + 0.0, the only sum below 1
    r = rolling.of(x[:7], None, 0, 2, "min")
    assert (r["best"], r["position"]) == (3.0, 0)             # 1 + 2 at 0, 2 + 1 at 2, 3 and 5: the first stays
    z = np.array([0.0, -0.0, 0.0])
    for which in ("max", "min"):                              # -0.0 == +0.0: the first window stays
        r = rolling.of(z, None, 0, 1, which)
        assert r["position"] == 0 and not np.signbit(r["best"])
    # a tie across a join: the earlier piece's window stays, also against the seam's
    a, b = rolling.of(x[:4], None, 0, 2), rolling.of(x[4:], None, 0, 2)
    m = rolling.merge(a, b)
    assert (m["best"], m["position"]) == (4.0, 1)
    same_records(m, rolling.of(x, None, 0, 2), "tie across the join")


def test_nan_and_infinities():
    inf, nan = np.inf, np.nan
    x = np.array([1.0, inf, 2.0, -inf, 5.0, nan, 100.0, 7.0])
    for which in ("max", "min"):
        r = rolling.of(x, None, 0, 2, which)                  # inf + 2 is no NaN; the NaN element gives the first NaN sum
        assert np.isnan(r["best"]) and r["position"] == 4 and r["n_windows"] == 7
        r = rolling.of(x, None, 0, 3, which)                  # +inf and -inf in one window: the first NaN sum
        assert np.isnan(r["best"]) and r["position"] == 1
        assert np.isnan(rolling.finalize(r, "mean").data) and not np.ma.getmaskarray(rolling.finalize(r)).any()
    r = rolling.of(x[:3], None, 0, 2, "max")
    assert r["best"] == inf and r["position"] == 0            # inf == inf: the first stays
    ok = np.ones(8, dtype=bool)
    ok[5] = False                                             # the NaN masked: it is no data any more
    r = rolling.of(x, ok, 0, 2, "max")
    assert r["best"] == inf and r["n_windows"] == 5 and r["n"] == 7
    # a NaN sum on either side of a join, and across it, wins in sequence order
    for cut in range(9):
        for w in (2, 3):
            m = rolling.merge(rolling.of(x[:cut], None, 0, w), rolling.of(x[cut:], None, 0, w))
            same_records(m, rolling.of(x, None, 0, w), ("nan", cut, w))


def test_mean_is_the_sum_divided_once():
    x = np.array([0.1, 0.2, 0.7, 0.3, 0.9, 0.4, 0.5], dtype=np.float32)
    for w in WINDOWS[:4]:
        r = rolling.of(x, None, 0, w)
        s = rolling.finalize(r, "sum").data
        assert rolling.finalize(r, "mean").data == s / np.float64(w)
    assert rolling.finalize(rolling.of(x, None, 0, 3)).data == \
        (np.float64(x[2]) + np.float64(x[3])) + np.float64(x[4])


def test_integers_convert_before_they_add():
    big = np.array([2 ** 60 + 1, 2 ** 60 + 129, 1, 2 ** 60 - 1], dtype=np.int64)
    r = rolling.of(big, None, 0, 2)
    f = big.astype(np.float64)
    assert r["best"] == f[0] + f[1] and r["position"] == 0
    assert f[0] == 2.0 ** 60 and f[1] == 2.0 ** 60 + 256.0    # each element rounds first


def test_module_argument_checks():
    assert rolling.check_window(np.int32(8)) == 8 and rolling.check_window(1) == 1
    for bad in (0, -1, 1.0, "3", None, True, np.True_):
        with pytest.raises(ValueError, match="window"):
            rolling.check_window(bad)
    for big in (9, 2 ** 40):
        with pytest.raises(NotImplementedError, match="more than 8"):
            rolling.check_window(big)
    with pytest.raises(ValueError, match="stat"):
        rolling.check_stat("max")
    with pytest.raises(ValueError, match="extreme"):
        rolling.check_extreme("sum")
    with pytest.raises(ValueError, match="valid_mask has shape"):
        rolling.of(np.zeros((2, 3)), np.ones((3, 2), bool), 0, 2)
    with pytest.raises(ValueError, match="along"):
        rolling.of(np.zeros((2, 3)), None, 2, 2)


# -- the Active API: every error before any device call --------------------------------
def test_api_returns_self_and_settings():
    a = Active(_var())
    assert a.rolling_path is None
    assert a.rolling(0, 5) is a and a._method == "rolling" and a._axis == (0,)
    assert a._rolling == {"along": 0, "window": 5, "stat": "sum", "which": "max"}
    assert a.method is None               # not one of the reference's methods
    assert a.rolling(-1, np.int64(3), stat="mean", extreme="min") is a
    assert a._rolling == {"along": 2, "window": 3, "stat": "mean", "which": "min"} and a._axis == (2,)
    a.method = "mean"
    assert a._rolling is None and a._method == "mean"
    a.rolling(1, 1)
    a.method = None
    assert a._rolling is None and a._method is None
    with pytest.raises(AttributeError):
        a.rolling_path = "cols"


@pytest.mark.parametrize("along", [3, -4, True, 1.0, "0", None])
def test_bad_along(no_device, along):
    a = Active(_var())
    with pytest.raises(ValueError, match="along"):
        a.rolling(along, 2)
    assert a._method is None and a._rolling is None


@pytest.mark.parametrize("kw, word", [
    (dict(window=0), "window"), (dict(window=-3), "window"), (dict(window=2.0), "window"),
    (dict(window=True), "window"), (dict(window=None), "window"), (dict(window="5"), "window"),
    (dict(stat="max"), "stat"), (dict(stat=None), "stat"), (dict(stat="SUM"), "stat"),
    (dict(extreme="sum"), "extreme"), (dict(extreme=None), "extreme"), (dict(extreme="Max"), "extreme")])
def test_bad_settings(no_device, kw, word):
    a = Active(_var())
    args = dict(window=2)
    args.update(kw)
    with pytest.raises(ValueError, match=f"rolling: {word}"):
        a.rolling(0, **args)
    assert a._method is None and a._rolling is None


@pytest.mark.parametrize("window", [9, 31, 2 ** 33])
def test_windows_past_the_cap(no_device, window):
    a = Active(_var())
    with pytest.raises(NotImplementedError, match="rolling: .*more than 8"):
        a.rolling(0, window)
    assert a._method is None and a._rolling is None


@pytest.mark.parametrize("index", [([1, 0],), ([0, 0, 1],), ([1, -2],), (np.array([1, 1]),),
                                   (slice(None, None, -1),), (1,)],
                         ids=["unsorted", "repeated", "negative-unsorted", "array-repeated", "negative-step", "int"])
def test_selection_along_must_keep_the_order(no_device, index):
    a = Active(_var())
    with pytest.raises(ValueError, match="rolling: the .* along dimension 0"):
        a.rolling(0, 2)[index]
    assert a._method is None and a._rolling is None              # cleared after the failed query


def test_kept_dims_take_any_list(no_device):
    a = Active(_var())
    with pytest.raises(AssertionError, match="a device call was made"):
        a.rolling(0, 2)[:, [2, 0], :]
    assert a._method is None and a._rolling is None


def test_weights_are_refused(no_device):
    a = Active(_var())
    a.weights = {0: [1.0, 2.0]}
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.rolling(0, 2)[...]
    assert a._rolling is None and a._weights is None and a._method is None


def test_group_not_implemented(no_device):
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="rolling with group="):
        a.rolling(0, 2)[...]
    assert a._rolling is None and a._method is None


def test_too_long_a_selection(no_device):
    n = 2 ** 31
    var = ChunkedVariable(name="v", shape=(n, 2), chunks=(2 ** 20, 2), dtype=np.dtype("|i1"), chunk_index={},
                          reader=lambda off, size: b"")
    a = Active(var)
    with pytest.raises(NotImplementedError, match="2\\^31"):
        a.rolling(0, 5)[...]
    assert a._rolling is None and a._method is None
