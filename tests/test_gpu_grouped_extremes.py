"""``Active.grouped("min" | "max" | "sum")`` on the device against NumPy.

Oracle: the selection taken with NumPy and masked with
``oracle.storage_ref.mask_missing``, kept in the variable's dtype; for each
group ``g`` it is restricted along ``along`` to the selected global indices
whose label is ``g`` and reduced with ``np.ma.min`` / ``np.ma.max`` /
``np.ma.sum`` (``keepdims=True``); the results are stacked along ``along``.

Masks, dtypes, shapes and NaN positions are exact.  ``min``, ``max`` and
integer ``sum`` are equal by ``==`` (either zero passes: the sign of a zero
extreme is not specified).  A float ``sum`` is held to the project's derived
bound against the exactly rounded sum of the group's values
(``_compare.exact_reference``): with ``B = sum_bound(float64, n, sum|x|)``,
``|got - exact| <= B`` for an f64 variable and ``B + 2^-24 (|exact| + B)`` for
an f32 one (its f64 sum is rounded to f32 once, at the end); where ``sum|x|``
is not finite the bound is 0: equality or a matching NaN.  Every float check
prints its largest error as a fraction of its bound; the largest over this
file, measured on an MI355X, is in DESIGN.md 6.14.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import _lib, engine, grouped
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes
from tests import _compare

pytestmark = pytest.mark.gpu

WORST = {"sum": 0.0}                  # the largest float-sum error seen, as a fraction of its bound
HUGE = 1e30                           # planted where nothing may be read
NP_FN = {"min": np.ma.min, "max": np.ma.max, "sum": np.ma.sum}


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
    if Ellipsis in index:
        k = index.index(Ellipsis)
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def _sum_dtype(dt):
    dt = np.dtype(dt).newbyteorder("=")
    return dt if dt.kind == "f" else np.dtype(np.int64 if dt.kind == "i" else np.uint64)


def oracle(data, attrs, labels, along, index, axis, n_groups):
    """Per group the masked selection, in the variable's dtype, restricted to
    the group's rows: ``n``, ``min``, ``max``, ``sum`` (NumPy's, in
    ``sum_dtype``), and for floats ``exact`` (the exactly rounded sum) and
    ``abs_sum``, each stacked along ``along``; plain arrays (masks follow from
    ``n``)."""
    index = _full_index(index, data.ndim)
    nat = data.dtype.newbyteorder("=")
    sel = ref.mask_missing(data[index], get_missing_attributes(attrs or {}))
    sel = np.ma.MaskedArray(np.ma.getdata(sel).astype(nat), mask=np.ma.getmaskarray(sel))
    lab = np.asarray(labels)[np.arange(data.shape[along])[index[along]]]
    red = tuple(range(data.ndim)) if axis is None else tuple(axis)
    shape1 = tuple(1 if d in red else n for d, n in enumerate(sel.shape))
    kinds = {"n": np.int64, "min": nat, "max": nat, "sum": _sum_dtype(nat), "exact": np.float64, "abs_sum": np.float64}
    out = {k: [] for k in kinds}
    for g in range(n_groups):
        rows = np.nonzero(lab == g)[0]
        if rows.size == 0 or 0 in shape1:
            for k in out:
                out[k].append(np.zeros(shape1, dtype=kinds[k]))
            continue
        sub = sel.take(rows, axis=along)
        with np.errstate(all="ignore"):
            out["n"].append((~np.ma.getmaskarray(sub)).sum(axis=red, keepdims=True))
            for stat in ("min", "max", "sum"):
                r = NP_FN[stat](sub, axis=red, keepdims=True)
                out[stat].append(np.ma.getdata(r).astype(kinds[stat]))
            if nat.kind == "f":
                ex = _compare.exact_reference(sub, axis=red)
                out["exact"].append(ex["exact"].reshape(shape1))
                out["abs_sum"].append(ex["abs_sum"].reshape(shape1))
            else:
                out["exact"].append(np.zeros(shape1))
                out["abs_sum"].append(np.zeros(shape1))
    if n_groups == 0:
        shape0 = tuple(0 if d == along else n for d, n in enumerate(shape1))
        return {k: np.zeros(shape0, dtype=kinds[k]) for k in out}
    return {k: np.concatenate(v, axis=along) for k, v in out.items()}


def float_sum_bound(o, dt):
    """The bound of a float sum per output (0 where sum|x| is not finite)."""
    with np.errstate(all="ignore"):
        B = _compare.sum_bound(np.float64, o["n"], o["abs_sum"])
        if np.dtype(dt).itemsize == 4:
            B = B + 2.0 ** -24 * (np.abs(o["exact"]) + B)
    return np.where(np.isfinite(o["abs_sum"]), B, 0.0)


def check(got, o, stat, dt, what=""):
    n = o["n"]
    nat = np.dtype(dt).newbyteorder("=")
    want_dt = _sum_dtype(nat) if stat == "sum" else nat
    assert isinstance(got, np.ma.MaskedArray), what
    assert got.dtype == want_dt and got.dtype.isnative and got.shape == n.shape, (what, got.dtype, got.shape, n.shape)
    m = np.ma.getmaskarray(got)
    assert m.shape == got.shape and np.array_equal(m, n == 0), what
    keep = ~m
    g = got.data[keep]
    if stat != "sum" or nat.kind != "f":
        w = o[stat][keep]
        if nat.kind == "f":
            assert np.array_equal(np.isnan(g), np.isnan(w)), (what, stat)
            assert np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)]), (what, stat)
        else:
            assert np.array_equal(g, w), (what, stat, g[g != w][:4], w[g != w][:4])
        return
    w, b = o["exact"][keep], float_sum_bound(o, nat)[keep]
    with np.errstate(all="ignore"):
        w = w.astype(np.float64)
        if nat.itemsize == 4:     # where the bound is 0 the f32 result is the exact sum's rounding (an infinity stays)
            w = np.where(b == 0, w.astype(np.float32).astype(np.float64), w)
    assert np.array_equal(np.isnan(g), np.isnan(w)), (what, "NaN positions")
    ratio = _compare.error_ratio(g, w, b)
    frac = float(ratio.max(initial=0.0))
    WORST["sum"] = max(WORST["sum"], frac)
    print(what, "sum: largest error as a fraction of its bound", frac, "(largest so far", WORST["sum"], ")")
    assert frac <= 1.0, (what, frac)


def query(var, stat, along, labels, axis, index, ddof=0, n_groups=None, components=False, **kw):
    a = Active(var, **kw)
    a.components = components
    got = a.grouped(stat, along, labels, axis=axis, ddof=ddof, n_groups=n_groups)[index]
    return got, a.grouped_path


def is_prefix(axis, ndim):
    return axis is not None and len(axis) < ndim and tuple(sorted(axis)) == tuple(range(len(axis)))


# -- label patterns ---------------------------------------------------------------
def cyclic(n):
    return np.arange(n) % 3, 3


def blocks(n):
    return np.arange(n) // 5, -(-n // 5)


def irregular(n):
    """Groups out of order, a gap (label 2 is absent) and excluded rows."""
    lab = np.random.default_rng(n).integers(-1, 5, n)
    lab[lab == 2] = 4
    lab[0], lab[n // 2], lab[-1] = 3, -1, 0
    return lab, 5


def roomy(n):
    """Two groups more than the labels need: masked outputs."""
    return np.arange(n) % 2, 4


PATTERNS = [cyclic, blocks, irregular, roomy]


# -- 1. sweep ---------------------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8", "<u8"]
INDEXES = [
    ("all", (Ellipsis,)),
    ("inner", (slice(1, -1), slice(1, -1), slice(1, -1))),
    ("stride", (slice(None), slice(None, None, 3), slice(None))),
    ("list", (slice(None), [0, 5, 6, 21], slice(None))),
    # [::-2, :, 3:30] as an index list (the planner takes slices of step >= 1 only)
    ("neg", (list(range(14, -1, -2)), slice(None), slice(3, 30))),
]
NUMPY_INDEX = {"neg": (slice(None, None, -2), slice(None), slice(3, 30))}
BOXES = ("all", "inner")
ALONG_AXIS = [(0, (0,)), (1, (0, 1)), (0, (0, 1)), (1, (1,)), (2, (2,)), (0, (0, 2)), (0, None)]
STATS = ["min", "max", "sum"]


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked, shuffle):
    """Noise about a plane; masked: 2 % fill values with valid_min / valid_max
    and a few values beyond them.  The chunks' padding holds 1e30 (floats) or
    a value beyond every datum."""
    d = np.dtype(dt)
    rng = np.random.default_rng(700 + DTYPES.index(dt))
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    if d.kind == "f":
        x = rng.normal(288.0, 10.0, SHAPE) + 0.8 * i0 - 0.3 * i1 + 0.1 * i2
        fill, lo, hi, pad = -999.0, 200.0, 380.0, HUGE
    elif d == np.dtype("<i8"):
        # beyond 2^53 in magnitude, about zero: a float64 comparison could not tell neighbours apart
        x = rng.integers(-2 ** 61, 2 ** 61, SHAPE, dtype=np.int64)
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 61) - 5, 2 ** 61 + 5
        pad = 2 ** 63 - 1
    elif d == np.dtype("<u8"):
        x = rng.integers(2 ** 63 - 1000, 2 ** 63 + 2 ** 61, SHAPE, dtype=np.uint64)
        fill, lo, hi = 2 ** 64 - 1, 2 ** 63 - 2000, 2 ** 63 + 2 ** 61 + 5
        pad = 0
    elif d == np.dtype("|u1"):
        x = rng.integers(10, 200, SHAPE) + 2 * i0 + i1
        fill, lo, hi, pad = 255, 5, 250, 255
    else:
        x = rng.integers(-3000, 3000, SHAPE) + 40 * i0 - 20 * i1 + 7 * i2
        fill, lo, hi, pad = -32768, -4100, 4100, 32767
    x = x.astype(d)
    attrs = {}
    if masked:
        f = x.reshape(-1)
        pos = rng.permutation(f.size)
        nf = f.size // 50
        f[pos[:nf]] = fill
        if d.kind == "f" or d == np.dtype("<i2"):
            f[pos[nf:nf + 20]] = d.type(lo - 50)
            f[pos[nf + 20:nf + 40]] = d.type(hi + 50)
        one = lambda v: np.array([v], dtype=d.newbyteorder("="))
        attrs = {"_FillValue": one(fill), "valid_min": one(lo), "valid_max": one(hi)}
    return x, attrs, make_var(x, CHUNKS, attrs, shuffle=shuffle, pad=pad)


def _sweep_cases():
    """Every dtype and index kind with two of the four (masked, shuffled)
    layouts, rotating so that every dtype meets all four."""
    k = 0
    for dt, (iname, index) in itertools.product(DTYPES, INDEXES):
        for masked, shuffle in (((False, False), (True, True)), ((True, False), (False, True)))[k % 2]:
            if shuffle and np.dtype(dt).itemsize == 1:
                shuffle = False   # the byte shuffle of 1-byte elements is the identity: no such layout
            yield dt, iname, index, masked, shuffle, k
        k += 1


def test_sweep(gpu):
    """Every dtype's index kinds and layouts; every (along, axis) pair; the
    statistic and the label pattern rotate.  (One test, and loops in place of
    parameters below: the suite's test count is kept down; the failing case
    is named in the assertion.)"""
    for dt, iname, index, masked, shuffle, k in _sweep_cases():
        x, attrs, var = sweep_var(dt, masked, shuffle)
        for j, (along, axis) in enumerate(ALONG_AXIS):
            stat = STATS[(k + j) % len(STATS)]
            pattern = PATTERNS[(k + 2 * j + int(masked)) % len(PATTERNS)]
            labels, n_g = pattern(SHAPE[along])
            got, path = query(var, stat, along, labels, axis, index, 0, n_g)
            what = (f"{dt} {iname} {'masked' if masked else 'plain'} {'shuffled' if shuffle else 'stored'} "
                    f"along {along} axis {axis} {pattern.__name__} {stat}")
            check(got, oracle(x, attrs, labels, along, NUMPY_INDEX.get(iname, index), axis, n_g), stat, dt, what)
            assert path == ("cols" if iname in BOXES and is_prefix(axis, 3) else "walk"), (what, path)


# -- 2. exactness in the variable's type ----------------------------------------------
def test_eight_byte_integers_are_exact(gpu):
    for index, path in (((Ellipsis,), "cols"), ((slice(None), slice(None, None, 2)), "walk")):
        _eight_byte_integers(index, path)


def _eight_byte_integers(index, path):
    labels = np.array([0, 1, 0, 1, 2, 2, 2, 0, 1])
    # <i8: extremes that differ only below bit 53, on both sides of zero; group 2 is three 2^62 (their sum wraps)
    x = np.full((9, 4, 8), 2 ** 60, dtype="<i8")
    x[1::2] = -(2 ** 60)
    x[2, 1, 3] = 2 ** 60 + 1
    x[3, 2, 5] = -(2 ** 60) - 1
    x[[4, 5, 6]] = 2 ** 62
    var = make_var(x, (4, 2, 4), pad=-(2 ** 63))
    o = oracle(x, None, labels, 0, index, (0,), 3)
    for stat in STATS:
        got, took = query(var, stat, 0, labels, (0,), index)
        assert took == path
        check(got, o, stat, "<i8", f"i8 {path} {stat}")
    mx, _ = query(var, "max", 0, labels, (0,), (Ellipsis,))
    mn, _ = query(var, "min", 0, labels, (0,), (Ellipsis,))
    sm, _ = query(var, "sum", 0, labels, (0,), (Ellipsis,))
    assert int(mx.data[0, 1, 3]) == 2 ** 60 + 1 and int(mx.data[0, 1, 2]) == 2 ** 60
    assert int(mn.data[1, 2, 5]) == -(2 ** 60) - 1 and int(mn.data[1, 2, 4]) == -(2 ** 60)
    assert (sm.data[2] == -(2 ** 62)).all() and int(np.full(3, 2 ** 62, dtype=np.int64).sum()) == -(2 ** 62)
    # <u8 above 2^63
    u = np.random.default_rng(5).integers(2 ** 63, 2 ** 64 - 1, (9, 4, 8), dtype=np.uint64).astype("<u8")
    u[0, 0, 0], u[2, 0, 0], u[7, 0, 0] = 2 ** 63 + 2, 2 ** 63 + 1, 2 ** 63 + 3
    uvar = make_var(u, (4, 2, 4), pad=0)
    ou = oracle(u, None, labels, 0, index, (0,), 3)
    for stat in STATS:
        got, took = query(uvar, stat, 0, labels, (0,), index)
        assert took == path
        check(got, ou, stat, "<u8", f"u8 {path} {stat}")
        if stat == "min":
            assert int(got.data[0, 0, 0]) == 2 ** 63 + 1


# -- 3. the dense path: aligned rows, runs, exclusion, the staging boundary -----------
@functools.lru_cache(maxsize=None)
def aligned_var(dt, shuffle=False):
    """Rows of 20 elements (a multiple of 4) in chunks whose bytes are a
    multiple of 16: whole-chunk queries take the 4-element loads."""
    rng = np.random.default_rng(62)
    shape, chunks = (26, 12, 40), (8, 6, 20)
    i0 = np.arange(26)[:, None, None]
    if np.dtype(dt).kind == "f":
        x = rng.normal(288.0, 10.0, shape) + 0.5 * i0
        pad = HUGE
    else:
        x = rng.integers(0, 200, shape) + i0
        pad = np.iinfo(np.dtype(dt)).max
    x = x.astype(dt)
    return x, make_var(x, chunks, shuffle=shuffle, pad=pad)


ALIGNED = [("<f4", False), ("<f4", True), (">f4", False), ("<f8", False), ("<f8", True), ("<i2", False), ("<i2", True),
           ("|u1", False), ("<i8", True), ("<u8", False)]


def test_aligned_rows_and_short_runs(gpu):
    """Runs of 2, 3, 5 and 16 rows scattered over the 26 time steps, whole and
    as a box that cuts the items at both ends."""
    labels = np.random.default_rng(8).permutation([0] * 2 + [1] * 3 + [2] * 5 + [3] * 16)
    for dt, shuffle in ALIGNED:
        x, var = aligned_var(dt, shuffle)
        name = f"aligned {dt} {'shuffled' if shuffle else 'stored'}"
        for index in ((Ellipsis,), (slice(2, 25), slice(1, 11), slice(3, 38))):
            o = oracle(x, None, labels, 0, index, (0,), 4)
            for stat in STATS:
                got, path = query(var, stat, 0, labels, (0,), index)
                assert path == "cols", name
                check(got, o, stat, dt, f"{name} {index} {stat}")
        got, path = query(var, "max", 1, np.arange(12) % 5, (0, 1), (Ellipsis,))
        assert path == "cols", name
        check(got, oracle(x, None, np.arange(12) % 5, 1, (Ellipsis,), (0, 1), 5), "max", dt, f"{name} along 1")


def test_excluded_rows_and_padding_are_not_read(gpu):
    """The rows of no group and the chunks' padding hold 1e30: one of them
    read as data would be the max and would swamp the sum."""
    labels = np.array([1, -1, 0, 0, -3, 1, 1, -1, -1, 2, 0, -1, 2, 2, 1, -1, 0, -1, -1, -1, 2, 1, 0, -1, -1, 2])
    for dt in ("<f4", "<f8"):
        x, _ = aligned_var(dt)
        x = x.copy()
        x[labels < 0] = HUGE
        var = make_var(x, (8, 6, 20), pad=HUGE)
        for index, path in (((Ellipsis,), "cols"), ((slice(1, 25), slice(None), slice(2, 39)), "cols"),
                            ((slice(None), slice(None, None, 2), slice(None)), "walk")):
            o = oracle(x, None, labels, 0, index, (0,), 3)
            for stat in STATS:
                got, took = query(var, stat, 0, labels, (0,), index)
                assert took == path, (dt, index)
                assert got.shape[0] == 3 and not np.ma.getmaskarray(got).any(), (dt, index)
                assert np.isfinite(got.data).all() and (stat == "sum" or float(got.max()) < 400.0), (dt, index, stat)
                assert float(got.max()) < 400.0 * 26, (dt, index, stat)
                check(got, o, stat, dt, f"excluded {dt} {path} {stat}")


def test_runs_across_and_on_the_staging_boundary(gpu):
    """More reduced rows than one staging pass holds: a run that crosses the
    pass boundary (its accumulators carry over) and a run that ends exactly on
    it (the next pass starts with a label change)."""
    R = _lib.GROUP_ROWS
    n = R + 37
    across = np.arange(n) // 93                        # run 11 is rows 1023 .. 1115
    assert across[R - 1] == across[R] == 11 and across[R - 2] == 10
    on = np.where(np.arange(n) < 930, np.arange(n) // 93, np.where(np.arange(n) < R, 10, 11))
    assert on[R - 1] == 10 and on[R] == 11 and (on == 10).sum() == 94
    for dt in ("|u1", "<f4"):
        rng = np.random.default_rng(17)
        x = (rng.integers(0, 250, (n, 2, 8)) if dt == "|u1" else rng.normal(10.0, 3.0, (n, 2, 8))).astype(dt)
        var = make_var(x, (64, 2, 8), pad=255 if dt == "|u1" else HUGE)
        for name, labels in (("across", across), ("on", on)):
            o = oracle(x, None, labels, 0, (Ellipsis,), (0,), 12)
            for stat in STATS:
                got, path = query(var, stat, 0, labels, (0,), (Ellipsis,))
                assert path == "cols" and got.shape == (12, 2, 8), (dt, name)
                check(got, o, stat, dt, f"staging {dt} {name} {stat}")


# -- 4. values ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_var():
    rng = np.random.default_rng(31)
    x = rng.normal(10.0, 3.0, (9, 12, 10)).astype("<f4")
    x[4, 5, 6] = np.nan                   # an unmasked NaN (group 1)
    x[6, 5, 7] = np.inf                   # +inf (group 0) and -inf (group 2) of one output
    x[2, 5, 7] = -np.inf
    x[0, 5, 8] = -np.inf                  # both in group 0 of another
    x[3, 5, 8] = np.inf
    x[[1, 4, 7], 7, 3] = -999.0           # group 1 of one output is all _FillValue
    x[:, 8, 2] = -999.0
    x[3, 8, 2] = 12.5                     # one counted element in group 0 of another
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    return x, attrs, make_var(x, (4, 6, 5), attrs, pad=-999.0)


VALUE_LABELS = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2])


def test_values(gpu):
    for index, path in (((Ellipsis,), "cols"), ((slice(None), slice(0, 12), [0, 2, 3, 4, 6, 7, 8]), "walk")):
        _values(index, path)


def _values(index, path):
    x, attrs, var = value_var()
    o = oracle(x, attrs, VALUE_LABELS, 0, index, (0,), 3)
    col = {0: 0, 2: 1, 3: 2, 4: 3, 6: 4, 7: 5, 8: 6} if path == "walk" else {k: k for k in range(10)}
    res = {}
    for stat in STATS:
        got, took = query(var, stat, 0, VALUE_LABELS, (0,), index)
        assert took == path
        check(got, o, stat, "<f4", f"values {path} {stat}")
        res[stat] = got
        m = np.ma.getmaskarray(got)
        assert m[1, 7, col[3]] and not m[0, 7, col[3]]                     # a group of fill values only: masked
        assert m[1, 8, col[2]] and m[2, 8, col[2]] and not m[0, 8, col[2]]
        assert got.data[0, 8, col[2]] == np.float32(12.5)                  # one element: min = max = sum
        nan = np.isnan(got.data) & ~m
        want = np.zeros_like(nan)
        want[1, 5, col[6]] = True                                          # the NaN's group, and only there ...
        if stat == "sum":
            want[0, 5, col[8]] = True                                      # ... and inf - inf in a sum
        assert np.array_equal(nan, want), stat
    assert res["max"].data[0, 5, col[7]] == np.inf and res["sum"].data[0, 5, col[7]] == np.inf
    assert res["min"].data[2, 5, col[7]] == -np.inf and res["sum"].data[2, 5, col[7]] == -np.inf
    assert res["min"].data[0, 5, col[8]] == -np.inf and res["max"].data[0, 5, col[8]] == np.inf


# -- 5. one group is the plain query -----------------------------------------------------
def test_single_group_is_the_plain_query(gpu):
    for dt in ("<f4", "<f8", "<i8", "<u8"):
        _single_group(dt)


def _single_group(dt):
    """(8-byte integers: the plain multi-chunk ``sum`` stores each chunk's sum
    in the variable's dtype before it combines them, as the reference does, so
    a 1- or 2-byte variable's plain sum wraps at that width where
    ``np.ma.sum`` and ``grouped`` do not; at 8 bytes both wrap modulo 2^64.)"""
    x, attrs, var = sweep_var(dt, True, False)
    zeros = np.zeros(15, dtype=np.int64)
    for index, axis, path in (((Ellipsis,), (0,), "cols"), ((slice(None), slice(None, None, 3)), (0, 2), "walk")):
        o = oracle(x, attrs, zeros, 0, index, axis, 1)
        for stat in STATS:
            got, took = query(var, stat, 0, zeros, axis, index)
            assert took == path
            plain = getattr(Active(var), stat)(axis=axis)[index]
            assert got.shape == plain.shape and got.dtype == plain.dtype, (stat, got.dtype, plain.dtype)
            assert np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(plain)), stat
            keep = ~np.ma.getmaskarray(got)
            if stat != "sum" or np.dtype(dt).kind != "f":
                assert np.array_equal(got.data[keep], np.ma.getdata(plain)[keep]), (dt, stat, path)
                continue
            # float sums: each within its own bound of the exact sum (the plain f64 query: sum_bound of its dtype)
            bg = float_sum_bound(o, dt)[keep]
            bp = _compare.sum_bound(np.dtype(dt).newbyteorder("="), o["n"], o["abs_sum"])[keep]
            err = np.abs(got.data[keep].astype(np.float64) - np.ma.getdata(plain)[keep].astype(np.float64))
            assert (err <= bg + bp).all(), (dt, path, float((err / (bg + bp)).max()))


# -- 6. components and merge -----------------------------------------------------------
def test_components_merge(gpu):
    for dt in ("<f4", "<i8"):
        _components_merge(dt)


def _components_merge(dt):
    x, attrs, var = sweep_var(dt, True, False)
    labels, n_g = cyclic(15)
    d = np.dtype(dt)

    def comps(index):
        got, path = query(var, "max", 0, labels, (0,), index, components=True)
        assert path == "cols"
        return got

    whole, lo, hi = comps(Ellipsis), comps(slice(0, 8)), comps(slice(8, None))
    assert sorted(whole) == ["max", "min", "n", "sum"]
    assert whole["n"].dtype == np.int64 and not np.ma.getmaskarray(whole["n"]).any()
    assert whole["sum"].dtype == (np.float64 if d.kind == "f" else np.int64)
    for k in ("sum", "min", "max"):
        assert whole[k].shape == (3, 22, 37) and (k == "sum" or whole[k].dtype == d.newbyteorder("="))
        assert np.array_equal(np.ma.getmaskarray(whole[k]), np.ma.getdata(whole["n"]) == 0)
    o = oracle(x, attrs, labels, 0, Ellipsis, (0,), n_g)
    np.testing.assert_array_equal(np.ma.getdata(whole["n"]), o["n"])

    def rec(c):
        r = np.zeros(c["n"].shape, dtype=engine.partial_dtype(d))
        r["count"] = np.ma.getdata(c["n"])
        for k in ("sum", "min", "max"):
            r[k] = np.ma.getdata(c[k])
        return r

    merged, w = grouped.merge_partials(rec(lo), rec(hi)), rec(whole)
    keep = w["count"] > 0
    np.testing.assert_array_equal(merged["count"], w["count"])
    for k in ("min", "max"):
        assert np.array_equal(merged[k][keep], w[k][keep]), k
        check(grouped.finalize(merged, k, dtype=d), o, k, dt, f"merged halves {k}")
    if d.kind == "f":
        B = _compare.sum_bound(np.float64, o["n"], o["abs_sum"])
        assert (np.abs(merged["sum"] - w["sum"])[keep] <= 2 * B[keep]).all()
    else:
        assert np.array_equal(merged["sum"], w["sum"])
    check(grouped.finalize(merged, "sum", dtype=d), o, "sum", dt, "merged halves sum")


# -- 7. determinism and residency ----------------------------------------------------------
def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


def test_deterministic_and_resident(gpu):
    for axis, index, path in (((0,), (slice(1, -1), slice(None), slice(2, 35)), "cols"),
                              ((0, 2), (slice(None), slice(None, None, 2), slice(None)), "walk")):
        _deterministic_and_resident(axis, index, path)


def _deterministic_and_resident(axis, index, path):
    x, attrs, var = sweep_var("<f4", True, True)
    labels, n_g = irregular(15)

    def run(resident, stat):
        a = Active(var, axis=axis, resident=resident)
        got = a.grouped(stat, 0, labels, n_groups=n_g)[index]
        assert a.grouped_path == path
        return got

    try:
        for stat in ("sum", "max"):
            first = run(False, stat)
            assert _bytes(run(False, stat)) == _bytes(first)
            assert _bytes(run(True, stat)) == _bytes(first)
            assert _bytes(run(True, stat)) == _bytes(first)
    finally:
        release_resident(var)
    assert var._pyas_resident is None


# -- 8. edges -------------------------------------------------------------------------
def test_edges(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    _, _, ivar = sweep_var("<i2", True, False)
    labels, n_g = cyclic(15)
    for stat, v, want in (("min", var, np.float32), ("max", ivar, np.int16), ("sum", var, np.float32),
                          ("sum", ivar, np.int64)):
        for index, shape in (((slice(0, 15), slice(5, 5), slice(None)), (3, 0, 37)), ((slice(4, 4),), (3, 22, 37))):
            a = Active(v)
            got = a.grouped(stat, 0, labels, axis=(0,))[index]
            assert isinstance(got, np.ma.MaskedArray) and got.dtype == want and got.shape == shape, (stat, index)
            assert np.ma.getmaskarray(got).shape == shape and np.ma.getmaskarray(got).all() and a.grouped_path is None
        a = Active(v)
        got = a.grouped(stat, 0, np.full(15, -1), axis=(0,))[...]                 # no group at all
        assert got.shape == (0, 22, 37) and got.dtype == want and a.grouped_path is None
        got = a.grouped(stat, 0, labels, axis=(0,), n_groups=None)[...]
        assert a.grouped_path == "cols"
        got0 = a.grouped(stat, 0, np.full(15, -1), axis=(0,), n_groups=0)[...]
        assert got0.shape == (0, 22, 37) and got0.dtype == want and a.grouped_path is None
        # every label negative but groups asked for: all masked, through the kernels
        for index, path in (((Ellipsis,), "cols"), ((slice(None, None, 2),), "walk")):
            neg = a.grouped(stat, 0, np.full(15, -1), axis=(0,), n_groups=2)[index]
            assert neg.shape == (2, 22, 37) and neg.dtype == want and np.ma.getmaskarray(neg).all()
            assert a.grouped_path == path
        # ddof is validated and ignored
        assert _bytes(a.grouped(stat, 0, labels, axis=(0,), ddof=3)[...]) == _bytes(got)
    a = Active(var, axis=(0,))
    with pytest.raises(ValueError, match="ddof"):
        a.grouped("max", 0, labels, ddof=-1)
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.weights = {0: np.ones(15)}
        a.grouped("sum", 0, labels)[...]
    assert a._weights is None and a._grouped is None
    with pytest.raises(ValueError, match="stat must be one of"):
        a.grouped("median", 0, labels)
    got = a.grouped("max", 0, labels)[...]
    assert a._method is None and a._grouped is None and a.grouped_path == "cols"   # the settings hold for one query
    check(got, oracle(x, attrs, labels, 0, Ellipsis, (0,), n_g), "max", "<f4", "after the errors")
    plain = a.max()[...]
    assert plain.shape == (1, 22, 37)


def teardown_module(module):
    print("test_gpu_grouped_extremes: largest float-sum error as a fraction of its bound:", WORST)
