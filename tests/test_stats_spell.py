"""``Active.spell`` on the device against NumPy.

Oracle: the selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``, converted with ``astype(float64)`` and
compared with the threshold; the runs along ``along`` counted by a Python loop
per output.  It shares nothing with ``pyactivestorage_amd/spell.py``.  Every
comparison is integer-exact.  ``spell_path`` is asserted in every case, so a
query that silently took the other kernel fails.
"""
import functools
import operator

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import spell
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

OPS = {"gt": operator.gt, "ge": operator.ge, "lt": operator.lt, "le": operator.le}
RECORD = ("n", "n_true", "len", "head", "tail", "best", "days", "events")
STATS = {"longest": "longest", "days": "days_total", "events": "events_total"}   # stat -> its components key


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


def _full_index(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    where = [k for k, s in enumerate(index) if s is Ellipsis]
    if where:
        k = where[0]
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def oracle(data, attrs, along, index, op, threshold, L, missing=None):
    """The record's fields and the three statistics per output (``along``
    kept with extent 1), by a run-length loop."""
    index = _full_index(index, data.ndim)
    ys = ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {}))
    valid = ~np.ma.getmaskarray(ys)
    with np.errstate(invalid="ignore"):
        true = OPS[op](np.ma.getdata(ys).astype(np.float64), threshold) & valid
    t2 = np.moveaxis(true, along, 0).reshape(true.shape[along], -1)
    v2 = np.moveaxis(valid, along, 0).reshape(true.shape[along], -1)
    T, n_out = t2.shape
    o = {k: np.zeros(n_out, dtype=np.int64) for k in RECORD + tuple(STATS.values())}
    for c in range(n_out):
        runs, start = [], None                      # (first position, length)
        for i in range(T):
            if t2[i, c] and start is None:
                start = i
            if not t2[i, c] and start is not None:
                runs.append((start, i - start))
                start = None
        if start is not None:
            runs.append((start, T - start))
        lens = [r for _, r in runs]
        o["n"][c], o["n_true"][c], o["len"][c] = v2[:, c].sum(), t2[:, c].sum(), T
        o["best"][c] = o["longest"][c] = max(lens, default=0)
        o["days_total"][c] = sum(r for r in lens if r >= L)
        o["events_total"][c] = sum(1 for r in lens if r >= L)
        o["head"][c] = runs[0][1] if runs and runs[0][0] == 0 else 0
        o["tail"][c] = runs[-1][1] if runs and runs[-1][0] + runs[-1][1] == T else 0
        inner = [r for s, r in runs if s > 0 and s + r < T and r >= L]
        o["days"][c], o["events"][c] = sum(inner), len(inner)
    shape = list(true.shape)
    shape[along] = 1
    kept = [s for d, s in enumerate(true.shape) if d != along]
    return {k: np.expand_dims(v.reshape(kept), along).reshape(shape) for k, v in o.items()}


def query(var, along, op, threshold, index, stat="longest", L=1, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = a.spell(along, op, threshold, stat=stat, min_length=L)[index]
    return got, a.spell_path


def check_stat(got, o, stat, what=""):
    assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.int64, what
    want = o[STATS[stat]]
    assert got.shape == want.shape, (what, got.shape, want.shape)
    wm = o["n"] == 0
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    assert np.array_equal(got.data[~wm], want[~wm]), (what, stat)


def check_components(comp, o, L, what=""):
    assert sorted(comp) == sorted(RECORD + ("min_length",) + tuple(STATS.values())), what
    for k in RECORD:
        assert comp[k].dtype == np.int64 and not np.ma.getmaskarray(comp[k]).any(), (what, k)
        assert np.array_equal(np.ma.getdata(comp[k]), o[k]), (what, k)
    assert (np.ma.getdata(comp["min_length"]) == L).all(), what
    for stat in STATS:
        check_stat(comp[STATS[stat]], o, stat, what)


def check_all(x, attrs, var, along, op, threshold, index, path, Ls=(1, 3, 6), what=""):
    """The three statistics for every L, and the components for the first."""
    for L in Ls:
        o = oracle(x, attrs, along, index, op, threshold, L)
        for stat in STATS:
            got, took = query(var, along, op, threshold, index, stat, L)
            assert took == path, (what, took)
            check_stat(got, o, stat, f"{what} {stat} L={L}")
    comp, took = query(var, along, op, threshold, index, L=Ls[0], components=True)
    assert took == path
    check_components(comp, oracle(x, attrs, along, index, op, threshold, Ls[0]), Ls[0], what)


HOT, COLD, THR = 30, 10, 20.0     # a true and a false value under ("gt", THR)


def pattern(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


# -- 1. the dense column kernel ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layers_var(dt="<f4", chunks=(5, 3, 8), shuffle=False, inner=8):
    """23 rows in layers of 5: runs cross layers, the padding of the last
    layer (rows 23, 24) holds values that satisfy the threshold."""
    p = pattern((23, 6, inner), 0.7, 5)
    p[:, 0, 0] = True                              # a run spanning the whole axis
    p[:, 0, 1] = False                             # an all-false column
    p[:, 0, 2] = False
    p[:3, 0, 2] = True                             # a run of exactly 3 at the very start
    p[:, 0, 3] = False
    p[-3:, 0, 3] = True                            # and at the very end
    p[:, 0, 4] = False
    p[5:10, 0, 4] = True                           # a wholly true middle layer
    p[:, 0, 5] = False
    p[:6, 0, 5] = p[-6:, 0, 5] = True              # runs of exactly 6 at both ends
    p[:, 1, 0] = True
    p[11, 1, 0] = False                            # two long runs
    x = np.where(p, HOT, COLD).astype(dt)
    return x, make_var(x, chunks, shuffle=shuffle, pad=HOT)


def test_cols_layers(gpu):
    x, var = layers_var()
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", what="layers")
    # the other three comparisons on the same data
    for op, thr in (("ge", 30.0), ("lt", 30.0), ("le", 10.0)):
        got, took = query(var, 0, op, thr, Ellipsis, "days", 3)
        assert took == "cols"
        check_stat(got, oracle(x, None, 0, Ellipsis, op, thr, 3), "days", op)


def test_cols_box_cuts_items(gpu):
    x, var = layers_var()
    index = (slice(3, 20), slice(1, None), slice(2, 7))
    check_all(x, None, var, 0, "gt", THR, index, "cols", what="box")
    index = (slice(3, 20), slice(0, 4), slice(5, 6))           # one output per row
    check_all(x, None, var, 0, "gt", THR, index, "cols", Ls=(3,), what="box of one")


def test_cols_rows_not_a_multiple_of_4(gpu):
    x, var = layers_var(chunks=(5, 3, 6), inner=11)
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", what="rows of 6")
    check_all(x, None, var, 0, "gt", THR, (slice(2, 22), slice(None), slice(1, 10)), "cols", Ls=(3,),
              what="rows of 6, box")


@pytest.mark.parametrize("dt", ["<f4", "<f8", "<i2"])
def test_cols_shuffled(gpu, dt):
    x, var = layers_var(dt=dt, shuffle=True)
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", Ls=(3,), what=f"shuffled {dt}")
    check_all(x, None, var, 0, "gt", THR, (slice(3, 20), slice(1, None), slice(2, 7)), "cols", Ls=(1,),
              what=f"shuffled {dt} box")


@pytest.mark.parametrize("dt", [">f4", ">i2", ">f8", ">u4"])
def test_cols_big_endian(gpu, dt):
    x, var = layers_var(dt=dt)
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", Ls=(3,), what=f"big-endian {dt}")


def test_cols_staging_pass(gpu):
    """1030-row layers: a run crosses the 1024-row staging pass and the layer
    boundary; run lengths that are no multiples of the 4 rows in flight."""
    rng = np.random.default_rng(9)
    p = np.zeros((2070, 2, 8), dtype=bool)
    for c in np.ndindex(2, 8):
        i = 0
        while i < 2070:
            r = int(rng.choice([1, 2, 3, 5, 6, 7, 9, 13]))     # a run, then a gap of 1 to 3
            p[i:i + r][(slice(None),) + c] = True
            i += r + int(rng.integers(1, 4))
    p[:, 0, 0] = False
    p[1000:1050, 0, 0] = True                                   # rows 1024 and 1030 inside the run
    p[2055:, 0, 0] = True                                       # 15 rows to the very end
    p[:, 0, 1] = True
    p[1029, 0, 1] = False
    x = np.where(p, HOT, COLD).astype("<f4")
    var = make_var(x, (1030, 2, 8), pad=HOT)
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", Ls=(6,), what="staging")
    check_all(x, None, var, 0, "gt", THR, (slice(1, 2069),), "cols", Ls=(3,), what="staging, cut")


DTYPES = ["|i1", "|u1", "<i2", "<u2", "<i4", "<u4", "<i8", "<u8", "<f4", "<f8"]


@pytest.mark.parametrize("dt", DTYPES)
def test_cols_dtypes(gpu, dt):
    """int64 / uint64: values 2^53 and more that differ from the threshold as
    integers but not after ``astype(float64)``, so the float64 rule decides."""
    d = np.dtype(dt)
    rng = np.random.default_rng(20 + DTYPES.index(dt))
    if d.itemsize == 8 and d.kind in "iu":
        e = 60 if d.kind == "i" else 63
        thr, op = 2.0 ** e, "ge"
        # 2^e - 1 rounds up to 2^e (true under ge, false as an integer); 2^e + 1 rounds down to it;
        # 2^e - 2^(e - 52) and 2^e - 2^(e - 53) - 1 are or round to the float64 below 2^e (false)
        vals = np.array([2 ** e - 1, 2 ** e + 1, 2 ** e - 2 ** (e - 52), 2 ** e - 2 ** (e - 53) - 1], dtype=d)
        assert (vals.astype(np.float64) >= thr).tolist() == [True, True, False, False]
        x = vals[rng.integers(0, 4, (23, 6, 8))]
    else:
        thr, op = THR, "gt"
        x = np.where(pattern((23, 6, 8), 0.7, 21), HOT, COLD).astype(d)
        if d.kind == "f":
            x[4, 2, 3] = np.nan
    var = make_var(x, (5, 3, 8), pad=np.nanmax(x))               # the padding satisfies the threshold
    check_all(x, None, var, 0, op, thr, Ellipsis, "cols", Ls=(2,), what=dt)
    check_all(x, None, var, 0, op, thr, (slice(1, 22), slice(1, 6), slice(1, 7)), "cols", Ls=(2,), what=f"{dt} box")


@functools.lru_cache(maxsize=None)
def masked_var():
    """Every element satisfies ("gt", THR); only the mask rules and the NaN
    break the runs."""
    x = np.full((23, 6, 8), 30.0, dtype="<f4")
    x[7, 0, 0] = 1000.0                            # _FillValue
    x[3, 0, 1] = 500.0                             # above valid_max
    x[12, 0, 2] = 22.0                             # below valid_min, still above the threshold
    x[9, 0, 3] = np.nan                            # compares false, counts as unmasked
    x[:, 0, 4] = 1000.0                            # a wholly masked column
    x[:, 0, 5] = 1000.0
    x[10:16, 0, 5] = 30.0                          # masked but for one run of 6
    x[5:11, 1, 0] = 500.0                          # a masked stretch across a layer boundary
    attrs = {"_FillValue": np.array([1000.0], "<f4"), "valid_min": np.array([25.0], "<f4"),
             "valid_max": np.array([400.0], "<f4")}
    return x, attrs, make_var(x, (5, 3, 8), attrs, pad=30.0)


def test_cols_mask_rules_break_runs(gpu):
    x, attrs, var = masked_var()
    check_all(x, attrs, var, 0, "gt", THR, Ellipsis, "cols", what="masked")
    got, _ = query(var, 0, "gt", THR, Ellipsis)
    assert np.ma.getmaskarray(got)[0, 0, 4] and np.ma.getmaskarray(got).sum() == 1
    assert got.data[0, 0, :4].tolist() == [15, 19, 12, 13] and got.data[0, 0, 5] == 6 and got.data[0, 1, 0] == 12
    comp, _ = query(var, 0, "gt", THR, Ellipsis, components=True)
    n = np.ma.getdata(comp["n"])
    assert n[0, 0, 3] == 23 and n[0, 0, 0] == 22 and n[0, 0, 4] == 0       # the NaN is unmasked
    # fill value only (mask mode: equality), and thresholds only (mask mode: range)
    for sub in ({"_FillValue": attrs["_FillValue"]}, {"valid_min": attrs["valid_min"], "valid_max": attrs["valid_max"]}):
        v = make_var(x, (5, 3, 8), sub, pad=30.0)
        check_all(x, sub, v, 0, "gt", THR, Ellipsis, "cols", Ls=(6,), what=f"masked {sorted(sub)}")


def test_components_merge_halves(gpu):
    x, var = layers_var()
    for L in (1, 3, 6):
        whole, _ = query(var, 0, "gt", THR, Ellipsis, L=L, components=True)
        lo, p1 = query(var, 0, "gt", THR, slice(0, 12), L=L, components=True)
        hi, p2 = query(var, 0, "gt", THR, slice(12, None), L=L, components=True)
        assert p1 == p2 == "cols"
        merged = spell.merge(lo, hi)
        for k in RECORD + ("min_length",):
            assert np.array_equal(merged[k], np.ma.getdata(whole[k])), (L, k)
        for stat in STATS:
            assert np.array_equal(spell.finalize(merged, stat), whole[STATS[stat]]), (L, stat)


# -- 2. the per-element walk -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def row_var(chunk):
    p = pattern((4, 150), 0.75, 31)
    p[0] = False
    p[0, 60:135] = True                            # crosses two 64-position words (and a chunk of 70)
    p[1] = True                                    # every position, every word
    p[2, 63:65] = False
    x = np.where(p, HOT, COLD).astype("<f4")
    return x, make_var(x, (4, chunk), pad=HOT)


@pytest.mark.parametrize("chunk", [150, 70])
def test_walk_innermost(gpu, chunk):
    x, var = row_var(chunk)
    check_all(x, None, var, 1, "gt", THR, Ellipsis, "walk", what=f"innermost, chunks of {chunk}")
    got, _ = query(var, -1, "gt", THR, Ellipsis)
    assert got.shape == (4, 1) and got.data[0, 0] == 75 and got.data[1, 0] == 150


@pytest.mark.parametrize("extent", [1, 63, 64, 65])
def test_walk_innermost_word_edges(gpu, extent):
    x, var = row_var(150)
    for start in (0, 58):
        index = (slice(None), slice(start, start + extent))
        check_all(x, None, var, 1, "gt", THR, index, "walk", Ls=(1, 6), what=f"extent {extent} from {start}")


@functools.lru_cache(maxsize=None)
def middle_var():
    x = np.where(pattern((5, 23, 7), 0.7, 41), HOT, COLD).astype("<i2")
    return x, make_var(x, (2, 5, 4), pad=HOT)


def test_walk_middle_dim(gpu):
    x, var = middle_var()
    check_all(x, None, var, 1, "gt", THR, Ellipsis, "walk", what="middle")
    check_all(x, None, var, 1, "gt", THR, (slice(1, 5), slice(2, 21), slice(1, 6)), "walk", Ls=(3,), what="middle box")
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "cols", Ls=(1,), what="middle var, along 0")


SELECTIONS = [
    ("stride", (slice(1, None, 3),)),
    ("list", ([0, 2, 3, 4, 9, 10, 11, 12, 13, 19, 22],)),
    ("bool", (np.arange(23) % 5 != 2,)),
    ("kept list", (slice(None), [4, 0, 5], slice(None))),
    ("kept stride", (slice(None), slice(None), slice(0, None, 2))),
]


@pytest.mark.parametrize("name,index", SELECTIONS, ids=[s[0].replace(" ", "-") for s in SELECTIONS])
def test_walk_selections(gpu, name, index):
    x, var = layers_var()
    check_all(x, None, var, 0, "gt", THR, index, "walk", Ls=(1, 3), what=name)
    x, attrs, var = masked_var()
    check_all(x, attrs, var, 0, "gt", THR, index, "walk", Ls=(6,), what=f"{name}, masked")


def test_walk_1d_two_fold_levels(gpu):
    """130 chunks of 7: the chunks' records fold in two levels of 64; runs
    cross chunks and the level boundary (chunk 64 starts at element 448)."""
    p = pattern((908,), 0.85, 51)
    p[438:441] = False
    p[441:460] = True
    p[460] = False
    p[896:] = True                                 # to the very end, in the cut last chunk
    x = np.where(p, HOT, COLD).astype("<f4")
    var = make_var(x, (7,), pad=HOT)
    check_all(x, None, var, 0, "gt", THR, Ellipsis, "walk", what="1-D")
    check_all(x, None, var, 0, "gt", THR, (slice(3, 900),), "walk", Ls=(6,), what="1-D cut")
    check_all(x, None, var, 0, "gt", THR, (slice(2, None, 2),), "walk", Ls=(3,), what="1-D stride")
    got, _ = query(var, 0, "gt", THR, Ellipsis)
    assert got.shape == (1,)


def test_vector_fill_value_takes_the_walk(gpu):
    x = np.full((20, 6, 10), 30.0, dtype="<f4")                # whole chunks: vector fill values need equal selections
    vec = np.array([31.0, 32.0, 33.0, 34.0, 35.0], "<f4")        # all above the threshold
    hit = pattern(x.shape, 0.15, 61)
    x[hit] = np.broadcast_to(np.tile(vec, 2), x.shape)[hit]
    var = make_var(x, (5, 3, 5), {"_FillValue": vec}, pad=30.0)
    missing = (np.tile(vec, 2), None, None, None)
    for along in (0, 2):
        o = oracle(x, None, along, Ellipsis, "gt", THR, 3, missing=missing)
        got, took = query(var, along, "gt", THR, Ellipsis, "days", 3)
        assert took == "walk"
        check_stat(got, o, "days", f"vector fill along {along}")


def test_empty_selection(gpu):
    x, var = layers_var()
    for index, shape in (((slice(4, 4),), (1, 6, 8)), ((slice(None), slice(5, 5)), (1, 0, 8))):
        a = Active(var)
        got = a.spell(0, "gt", THR)[index]
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.int64 and got.shape == shape
        assert np.ma.getmaskarray(got).all() and a.spell_path is None
        a.components = True
        comp = a.spell(0, "gt", THR, stat="days", min_length=3)[index]
        assert comp["longest"].shape == shape and comp["n"].shape == shape and comp["n"].dtype == np.int64


# -- 3. both paths, run to run ---------------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


def test_both_paths_agree(gpu):
    """``[0:T]`` (the column kernel) against the explicit list ``arange(T)``
    and a full boolean mask (the walk): the same records."""
    for (x, attrs, var) in ((*layers_var()[:1], None, layers_var()[1]), masked_var()):
        T = x.shape[0]
        cols, p0 = query(var, 0, "gt", THR, (slice(0, T),), L=3, components=True)
        assert p0 == "cols"
        for index in ((list(range(T)),), (np.ones(T, dtype=bool),)):
            walk, p1 = query(var, 0, "gt", THR, index, L=3, components=True)
            assert p1 == "walk"
            for k in cols:
                assert _bytes(cols[k]) == _bytes(walk[k]), k


@pytest.mark.parametrize("index,path", [((Ellipsis,), "cols"), ((slice(1, None, 2),), "walk")], ids=["cols", "walk"])
def test_deterministic(gpu, index, path):
    x, attrs, var = masked_var()
    first, took = query(var, 0, "gt", THR, index, "days", 3)
    assert took == path
    for _ in range(2):
        again, _ = query(var, 0, "gt", THR, index, "days", 3)
        assert _bytes(again) == _bytes(first)


def test_settings_hold_for_one_query(gpu):
    x, var = layers_var()
    a = Active(var)
    got = a.spell(0, "gt", THR, stat="events", min_length=3)[...]
    assert a._method is None and a._spell is None and a.spell_path == "cols"
    check_stat(got, oracle(x, None, 0, Ellipsis, "gt", THR, 3), "events", "first")
    mean = a.mean()[...]                                          # the next query is a plain mean over axis 0
    assert mean.shape == (1, 6, 8) and a.spell_path == "cols"
    with pytest.raises(ValueError, match="strictly increasing"):
        a.spell(0, "gt", THR)[[3, 1]]
    assert a._spell is None and a._method is None
