"""``Active.grouped`` on the device against NumPy.

Oracle: the selection taken with NumPy, masked with
``oracle.storage_ref.mask_missing`` and converted to float64; for each group
``g`` it is restricted along ``along`` to the selected global indices whose
label is ``g`` and reduced with ``np.ma.mean`` / ``np.ma.var`` / ``np.ma.std``
(``keepdims=True``) or counted; the results are stacked along ``along``.

Tolerances, from the project's own:

* ``var`` / ``std``: ``RTOL = 1e-9`` relative, the bound of
  ``tests/test_gpu_moments.py`` (the same accumulator and merge; a record
  covers fewer elements).
* ``mean``: ``|got - want| <= 1e-9 (|want| + sigma)``, ``sigma`` the oracle's
  population standard deviation of that output: the shifted sum errs by about
  ``n_lane 2^-53`` of the spread, and a record carries its mean as one f64, so
  a merge costs about ``2^-53 (|mean| + spread)``.

Masks, counts and NaN positions are exact (a group that counts a NaN or an
infinity is NaN in every statistic); dtypes and shapes are exact.  Every check
prints its largest error as a fraction of its bound; the largest over this
file, measured on an MI355X, are in DESIGN.md 6.13.
"""
import functools
import itertools

import numpy as np
import pytest

from oracle import storage_ref as ref
from pyactivestorage_amd import _lib, moments
from pyactivestorage_amd.active import Active, release_resident
from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes

pytestmark = pytest.mark.gpu

RTOL = 1e-9                           # the project's second-moment bound
WORST = {"mean": 0.0, "var": 0.0, "std": 0.0}   # the largest errors seen, as fractions of the bounds above
HUGE = 1e30                           # planted where nothing may be read: one element of it would show in any mean


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


def oracle(data, attrs, labels, along, index, axis, n_groups, missing=None):
    """Per group the float64 masked selection restricted to the group's rows:
    ``n``, ``mean``, ``var`` (ddof 0 and 1) and ``bad`` (the group counts a
    NaN or an infinity: np.ma masks such a mean, the device gives NaN), each
    stacked along ``along``; plain arrays (masks follow from ``n``)."""
    index = _full_index(index, data.ndim)
    sel = ref.mask_missing(data[index], missing or get_missing_attributes(attrs or {}))
    x64 = np.ma.MaskedArray(np.ma.getdata(sel).astype(np.float64), mask=np.ma.getmaskarray(sel))
    lab = np.asarray(labels)[np.arange(data.shape[along])[index[along]]]     # the selected global indices' labels
    red = tuple(range(data.ndim)) if axis is None else tuple(axis)
    shape1 = tuple(1 if d in red else n for d, n in enumerate(x64.shape))
    out = {k: [] for k in ("n", "mean", "var0", "var1", "bad")}
    kind = {"n": np.int64, "bad": bool}
    for g in range(n_groups):
        rows = np.nonzero(lab == g)[0]
        if rows.size == 0:
            for k in out:
                out[k].append(np.zeros(shape1, dtype=kind.get(k, np.float64)))
            continue
        sub = x64.take(rows, axis=along)
        with np.errstate(all="ignore"):
            out["n"].append((~np.ma.getmaskarray(sub)).sum(axis=red, keepdims=True))
            out["bad"].append((~np.ma.getmaskarray(sub) & ~np.isfinite(np.ma.getdata(sub))).any(axis=red, keepdims=True))
            out["mean"].append(np.ma.getdata(sub.mean(axis=red, keepdims=True)).astype(np.float64))
            out["var0"].append(np.ma.getdata(sub.var(axis=red, ddof=0, keepdims=True)).astype(np.float64))
            out["var1"].append(np.ma.getdata(sub.var(axis=red, ddof=1, keepdims=True)).astype(np.float64))
    if n_groups == 0:
        shape0 = tuple(0 if d == along else n for d, n in enumerate(shape1))
        return {k: np.zeros(shape0, dtype=kind.get(k, np.float64)) for k in out}
    return {k: np.concatenate(v, axis=along) for k, v in out.items()}


def check(got, o, stat, ddof=0, what=""):
    n = o["n"]
    if stat == "count":
        assert type(got) is np.ndarray and got.dtype == np.int64 and got.shape == n.shape, what
        assert np.array_equal(got, n), what
        return
    assert isinstance(got, np.ma.MaskedArray), what
    assert got.dtype == np.float64 and got.shape == n.shape, (what, got.shape, n.shape)
    wm = n == 0 if stat == "mean" else n - ddof <= 0
    assert np.array_equal(np.ma.getmaskarray(got), wm), what
    with np.errstate(all="ignore"):
        sigma = np.sqrt(o["var0"])
        if stat == "mean":
            want, bound = o["mean"], RTOL * (np.abs(o["mean"]) + sigma)
        else:
            want = o[f"var{ddof}"]
            want = np.sqrt(want) if stat == "std" else want
            bound = RTOL * np.abs(want)
    nan = o["bad"][~wm]                         # a counted NaN or infinity
    g, w, b = got.data[~wm], want[~wm], bound[~wm]
    assert np.array_equal(np.isnan(g), nan), (what, int(np.isnan(g).sum()), int(nan.sum()))
    err, bb = np.abs(g[~nan] - w[~nan]), b[~nan]
    ok = err <= bb
    frac = float((err[bb > 0] / bb[bb > 0]).max(initial=0.0))
    WORST[stat] = max(WORST[stat], frac)
    print(what, stat, "largest error as a fraction of its bound", frac, "(largest so far", WORST[stat], ")")
    assert ok.all(), (what, stat, float(err[~ok].max()), float(bb[~ok].min()))


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
DTYPES = ["<f4", ">f4", "<f8", "<i2", "|u1", "<i8"]
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
STATS = [("mean", 0), ("var", 0), ("std", 1), ("var", 1), ("count", 0), ("std", 0)]


@functools.lru_cache(maxsize=None)
def sweep_var(dt, masked, shuffle):
    """Noise about a plane; masked: 2 % fill values with valid_min / valid_max
    and a few values beyond them.  The chunks' padding holds 1e30 (floats) or
    the fill value."""
    d = np.dtype(dt)
    rng = np.random.default_rng(500 + DTYPES.index(dt))
    i0, i1, i2 = np.meshgrid(*[np.arange(n) for n in SHAPE], indexing="ij")
    if d.kind == "f":
        x = rng.normal(288.0, 10.0, SHAPE) + 0.8 * i0 - 0.3 * i1 + 0.1 * i2
        fill, lo, hi, pad = -999.0, 200.0, 380.0, HUGE
    elif d == np.dtype("<i8"):
        # odd values up to 2^56 in magnitude, spread about zero (tests/test_gpu_moments.py)
        x = rng.integers(-2 ** 55, 2 ** 55, SHAPE) * 2 + 1
        fill, lo, hi = -(2 ** 62) - 1, -(2 ** 60), 2 ** 60
        pad = fill
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


@pytest.mark.parametrize("dtype", DTYPES, ids=[d.replace("|", "=") for d in DTYPES])
def test_sweep(gpu, dtype):
    """One dtype's index kinds and layouts (one test per dtype keeps the
    suite's test count down; the failing case is named in the assertion).
    Every (along, axis) pair; the statistic and the label pattern rotate."""
    for dt, iname, index, masked, shuffle, k in _sweep_cases():
        if dt != dtype:
            continue
        x, attrs, var = sweep_var(dt, masked, shuffle)
        for j, (along, axis) in enumerate(ALONG_AXIS):
            stat, ddof = STATS[(k + j) % len(STATS)]
            pattern = PATTERNS[(k + 2 * j + int(masked)) % len(PATTERNS)]
            labels, n_g = pattern(SHAPE[along])
            got, path = query(var, stat, along, labels, axis, index, ddof, n_g)
            what = (f"{dt} {iname} {'masked' if masked else 'plain'} {'shuffled' if shuffle else 'stored'} "
                    f"along {along} axis {axis} {pattern.__name__}")
            check(got, oracle(x, attrs, labels, along, NUMPY_INDEX.get(iname, index), axis, n_g), stat, ddof, what)
            assert path == ("cols" if iname in BOXES and is_prefix(axis, 3) else "walk"), (what, path)


# -- 2. the dense path: aligned rows, runs, exclusion, the staging boundary -----------
@functools.lru_cache(maxsize=None)
def aligned_var(dt, shuffle=False):
    """Rows of 20 elements (a multiple of 4) in chunks whose bytes are a
    multiple of 16: whole-chunk queries take the 4-element loads."""
    rng = np.random.default_rng(61)
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
           ("|u1", False), ("<i8", True)]


def test_aligned_rows_and_short_runs(gpu):
    """Runs of 2, 3, 5 and 16 rows scattered over the 26 time steps (no run
    of the short ones is a multiple of the 4-row fetch), whole and as a box
    that cuts the items at both ends."""
    labels = np.random.default_rng(8).permutation([0] * 2 + [1] * 3 + [2] * 5 + [3] * 16)
    for dt, shuffle in ALIGNED:
        x, var = aligned_var(dt, shuffle)
        name = f"aligned {dt} {'shuffled' if shuffle else 'stored'}"
        for index in ((Ellipsis,), (slice(2, 25), slice(1, 11), slice(3, 38))):
            for stat, ddof in (("mean", 0), ("var", 1)):
                got, path = query(var, stat, 0, labels, (0,), index, ddof)
                assert path == "cols", name
                check(got, oracle(x, None, labels, 0, index, (0,), 4), stat, ddof, f"{name} {index}")
        got, path = query(var, "std", 1, np.arange(12) % 5, (0, 1), (Ellipsis,))
        assert path == "cols", name
        check(got, oracle(x, None, np.arange(12) % 5, 1, (Ellipsis,), (0, 1), 5), "std", 0, f"{name} along 1")


def test_excluded_rows_are_not_read(gpu):
    """The rows of no group hold 1e30: one of them read as data would show in
    every mean.  Unmasked data, so nothing else would hide it."""
    labels = np.array([1, -1, 0, 0, -3, 1, 1, -1, -1, 2, 0, -1, 2, 2, 1, -1, 0, -1, -1, -1, 2, 1, 0, -1, -1, 2])
    for dt in ("<f4", "<f8"):
        x, _ = aligned_var(dt)
        x = x.copy()
        x[labels < 0] = HUGE
        var = make_var(x, (8, 6, 20), pad=HUGE)
        for index, path in (((Ellipsis,), "cols"), ((slice(1, 25), slice(None), slice(2, 39)), "cols"),
                            ((slice(None), slice(None, None, 2), slice(None)), "walk")):
            got, took = query(var, "mean", 0, labels, (0,), index)
            assert took == path, (dt, index)
            assert got.shape[0] == 3 and not np.ma.getmaskarray(got).any() and float(got.max()) < 400.0, (dt, index)
            check(got, oracle(x, None, labels, 0, index, (0,), 3), "mean", 0, f"excluded {dt} {path}")


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
            for stat in ("mean", "var"):
                got, path = query(var, stat, 0, labels, (0,), (Ellipsis,))
                assert path == "cols" and got.shape == (12, 2, 8), (dt, name)
                check(got, oracle(x, None, labels, 0, (Ellipsis,), (0,), 12), stat, 0, f"staging {dt} {name}")
            cnt, _ = query(var, "count", 0, labels, (0,), (Ellipsis,))
            check(cnt, oracle(x, None, labels, 0, (Ellipsis,), (0,), 12), "count", 0, f"staging {dt} {name}")


# -- 3. values ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_var():
    rng = np.random.default_rng(31)
    x = rng.normal(10.0, 3.0, (9, 12, 10)).astype("<f4")
    x[4, 5, 6] = np.nan                   # an unmasked NaN (group 1)
    x[6, 5, 7] = np.inf                   # an infinity, not the first of its group's run (group 0)
    x[0, 5, 8] = -np.inf                  # and one that is (group 0)
    x[[1, 4, 7], 7, 3] = -999.0           # group 1 of one output is all _FillValue
    x[:, 8, 2] = -999.0
    x[3, 8, 2] = 12.5                     # one counted element in group 0 of another
    attrs = {"_FillValue": np.array([-999.0], "<f4")}
    return x, attrs, make_var(x, (4, 6, 5), attrs, pad=-999.0)


VALUE_LABELS = np.array([0, 1, 2, 0, 1, 2, 0, 1, 2])


@pytest.mark.parametrize("index,path", [((Ellipsis,), "cols"), ((slice(None), slice(0, 12), [0, 2, 3, 4, 6, 7, 8]),
                                                               "walk")], ids=["cols", "walk"])
def test_values(gpu, index, path):
    x, attrs, var = value_var()
    o = oracle(x, attrs, VALUE_LABELS, 0, index, (0,), 3)
    col = {0: 0, 2: 1, 3: 2, 4: 3, 6: 4, 7: 5, 8: 6} if path == "walk" else {k: k for k in range(10)}
    for stat, ddof in (("mean", 0), ("var", 0), ("std", 1), ("count", 0)):
        got, took = query(var, stat, 0, VALUE_LABELS, (0,), index, ddof)
        assert took == path
        check(got, o, stat, ddof, f"values {path}")
        if stat == "count":
            assert got[1, 7, col[3]] == 0 and got[0, 8, col[2]] == 1 and got[1, 8, col[2]] == 0
            continue
        m = np.ma.getmaskarray(got)
        assert m[1, 7, col[3]] and not m[0, 7, col[3]]                     # a group of fill values only: masked
        assert m[1, 8, col[2]] and m[2, 8, col[2]]
        assert m[0, 8, col[2]] == (stat == "std")                          # one element: var 0, std with ddof 1 masked
        if stat == "mean":
            assert got.data[0, 8, col[2]] == 12.5
        elif stat == "var":
            assert got.data[0, 8, col[2]] == 0.0
        nan = np.isnan(got.data) & ~m
        want = np.zeros_like(nan)
        want[1, 5, col[6]] = want[0, 5, col[7]] = want[0, 5, col[8]] = True   # NaN at those outputs only
        assert np.array_equal(nan, want), stat


def test_single_group_is_the_plain_variance(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    zeros = np.zeros(15, dtype=np.int64)
    for index, axis, path in (((Ellipsis,), (0,), "cols"), ((slice(None), slice(None, None, 3)), (0, 2), "walk")):
        sel = ref.mask_missing(x[_full_index(index, 3)], get_missing_attributes(attrs)).astype(np.float64)
        for stat, fn in (("var", np.ma.var), ("std", np.ma.std), ("mean", np.ma.mean)):
            got, took = query(var, stat, 0, zeros, axis, index, ddof=0)
            assert took == path
            want = fn(sel, axis=axis, keepdims=True)
            assert got.shape == want.shape and np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))
            np.testing.assert_allclose(got.compressed(), want.compressed(), rtol=RTOL, atol=0)
        plain = Active(var).var(axis=axis)[index]
        got, _ = query(var, "var", 0, zeros, axis, index)
        np.testing.assert_allclose(got.compressed(), plain.compressed(), rtol=RTOL, atol=0)


def test_selection_along_uses_its_global_indices(gpu):
    x, attrs, var = sweep_var("<f8", True, False)
    labels, n_g = irregular(15)
    for index in ((slice(1, None, 3),), ([13, 2, 3, 9, 0],)):   # a stride and a list along the labelled dim
        for axis in ((0,), (0, 2), None):
            got, path = query(var, "mean", 0, labels, axis, index, n_groups=n_g)
            assert path == "walk", (index, axis)
            check(got, oracle(x, attrs, labels, 0, index, axis, n_g), "mean", 0, f"along selection {index} {axis}")


def test_vector_fill_value_takes_the_walk(gpu):
    rng = np.random.default_rng(41)
    a = rng.normal(10.0, 3.0, (8, 6, 10)).astype("<f4") + np.arange(10, dtype="<f4")
    vec = np.array([1.0, 2.0, 3.0, 4.0, 5.0], "<f4")
    hit = rng.random(a.shape) < 0.1
    a[hit] = np.broadcast_to(np.tile(vec, 2), a.shape)[hit]
    var = make_var(a, (4, 3, 5), {"_FillValue": vec})
    for axis in (None, (0,), (2,)):
        along = 2 if axis == (2,) else 0
        labels = np.array([1, 0, -1, 1, 0, 2, 2, 1, 0, 1])[:a.shape[along]]
        for stat in ("mean", "var", "count"):
            got, path = query(var, stat, along, labels, axis, Ellipsis)
            assert path == "walk", axis
            check(got, oracle(a, None, labels, along, Ellipsis, axis, 3, missing=(np.tile(vec, 2), None, None, None)),
                  stat, 0, f"vector fill axis {axis}")


# -- 4. other behaviour -------------------------------------------------------------
def test_zero_size_selection_and_no_group(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    labels, _ = cyclic(15)
    for index, shape in (((slice(0, 15), slice(5, 5), slice(None)), (3, 0, 37)), ((slice(4, 4),), (3, 22, 37))):
        a = Active(var)
        got = a.grouped("mean", 0, labels, axis=(0,))[index]
        assert isinstance(got, np.ma.MaskedArray) and got.dtype == np.float64 and got.shape == shape
        assert np.ma.getmaskarray(got).all() and a.grouped_path is None
        cnt = a.grouped("count", 0, labels, axis=(0,))[index]
        assert type(cnt) is np.ndarray and cnt.dtype == np.int64 and cnt.shape == shape and not cnt.any()
        a.components = True
        comp = a.grouped("var", 0, labels, axis=(0,))[index]
        assert sorted(comp) == ["m2", "mean", "n"] and comp["n"].shape == shape and comp["n"].dtype == np.int64
    a = Active(var)
    got = a.grouped("var", 0, np.full(15, -1), axis=(0,))[...]
    assert got.shape == (0, 22, 37) and got.dtype == np.float64 and a.grouped_path is None
    # every label negative but groups asked for: all masked, through the kernels
    for index, path in (((Ellipsis,), "cols"), ((slice(None, None, 2),), "walk")):
        got = a.grouped("mean", 0, np.full(15, -1), axis=(0,), n_groups=2)[index]
        assert got.shape == (2, 22, 37) and np.ma.getmaskarray(got).all() and a.grouped_path == path


def test_components_merge(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    labels, n_g = cyclic(15)

    def comps(index):
        got, path = query(var, "var", 0, labels, (0,), index, components=True)
        assert path == "cols"
        return got

    whole, lo, hi = comps(Ellipsis), comps(slice(0, 8)), comps(slice(8, None))
    assert sorted(whole) == ["m2", "mean", "n"]
    assert whole["n"].dtype == np.int64 and not np.ma.getmaskarray(whole["n"]).any()
    for k in ("mean", "m2"):
        assert whole[k].dtype == np.float64 and whole[k].shape == (3, 22, 37)
        assert np.array_equal(np.ma.getmaskarray(whole[k]), np.ma.getdata(whole["n"]) == 0)
    o = oracle(x, attrs, labels, 0, Ellipsis, (0,), n_g)
    np.testing.assert_array_equal(np.ma.getdata(whole["n"]), o["n"])
    rec = lambda c: moments.records(np.ma.getdata(c["n"]), np.ma.getdata(c["mean"]), np.ma.getdata(c["m2"]))
    merged = moments.merge(rec(lo), rec(hi))
    np.testing.assert_array_equal(merged["count"], np.ma.getdata(whole["n"]))
    check(moments.finalize(merged, 0), o, "var", 0, "merged halves")
    check(moments.finalize(rec(whole), 1, std=True), o, "std", 1, "whole")
    np.testing.assert_allclose(merged["mean"], np.ma.getdata(whole["mean"]), rtol=RTOL)
    np.testing.assert_allclose(merged["m2"], np.ma.getdata(whole["m2"]), rtol=RTOL)


def _bytes(r):
    return np.ma.getdata(r).tobytes() + np.ma.getmaskarray(r).tobytes()


@pytest.mark.parametrize("axis,index,path", [((0,), (slice(1, -1), slice(None), slice(2, 35)), "cols"),
                                             ((0, 2), (slice(None), slice(None, None, 2), slice(None)), "walk")],
                         ids=["cols", "walk"])
def test_deterministic_and_resident(gpu, axis, index, path):
    x, attrs, var = sweep_var("<f4", True, True)
    labels, n_g = irregular(15)

    def run(resident):
        a = Active(var, axis=axis, resident=resident)
        got = a.grouped("var", 0, labels, n_groups=n_g)[index]
        assert a.grouped_path == path
        return got

    first = run(False)
    assert _bytes(run(False)) == _bytes(first)
    try:
        assert _bytes(run(True)) == _bytes(first)
        assert _bytes(run(True)) == _bytes(first)
    finally:
        release_resident(var)
    assert var._pyas_resident is None


def test_settings_hold_for_one_query(gpu):
    x, attrs, var = sweep_var("<f4", True, False)
    labels, n_g = cyclic(15)
    a = Active(var, axis=(0,))
    got = a.grouped("mean", 0, labels)[...]
    assert a._method is None and a._grouped is None and a.grouped_path == "cols"
    check(got, oracle(x, attrs, labels, 0, Ellipsis, (0,), n_g), "mean", 0, "first")
    mean = a.mean()[...]                                         # the next query is a plain mean
    assert mean.shape == (1, 22, 37) and a.grouped_path == "cols"
    with pytest.raises(ValueError, match="not among the reduced axes"):
        a.grouped("mean", 1, np.zeros(22, dtype=int))[...]       # the object's axis is still (0,)
    assert a._grouped is None
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.weights = {0: np.ones(15)}
        a.grouped("mean", 0, labels)[...]
    assert a._weights is None
    b = Active(var, axis=(0,), group=object())
    with pytest.raises(NotImplementedError, match="grouped with group="):
        b.grouped("mean", 0, labels)[...]
    var1 = a.grouped("var", 0, labels, ddof=1)[...]
    check(var1, oracle(x, attrs, labels, 0, Ellipsis, (0,), n_g), "var", 1, "ddof 1")
    var0 = a.var()[...]                                          # ddof does not stick
    assert var0.shape == (1, 22, 37) and a._ddof == 0


def teardown_module(module):
    print("test_gpu_grouped: largest errors as fractions of the bounds:", WORST)
