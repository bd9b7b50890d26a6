"""``pyactivestorage_amd.histogram`` on the host: edge validation, the NumPy
statement of the bin rule against ``np.histogram`` of float64 data, ``merge``
and ``quantile``.  All count comparisons are exact."""
import numpy as np
import pytest

from pyactivestorage_amd import histogram as H
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable


# -- edges ---------------------------------------------------------------------
def test_edges_of_a_count_are_linspace():
    for n, lo, hi in [(1, 0.0, 1.0), (7, 270.1, 305.3), (64, 256, 320), (2048, -1e300, 1e300), (3, -5, -5 + 1e-9)]:
        e = H.edges(n, (lo, hi))
        assert e.dtype == np.float64 and e.shape == (n + 1,)
        assert np.array_equal(e, np.linspace(lo, hi, n + 1))
        assert np.array_equal(e, np.histogram_bin_edges(np.zeros(0), bins=n, range=(lo, hi)))
    assert np.array_equal(H.edges(np.int32(4), (np.float32(1), 3)), np.linspace(1, 3, 5))


@pytest.mark.parametrize("v", [0.0, 288.0, -3.5, 1e12])
def test_equal_range_ends_widen_by_a_half(v):
    e = H.edges(5, (v, v))
    assert np.array_equal(e, np.linspace(v - 0.5, v + 0.5, 6))
    assert np.array_equal(e, np.histogram_bin_edges(np.zeros(0), bins=5, range=(v, v)))


def test_edges_of_a_sequence():
    e = H.edges([1, 2.5, 4, 100])
    assert e.dtype == np.float64 and np.array_equal(e, [1.0, 2.5, 4.0, 100.0])
    src = np.array([0.0, 1.0])
    out = H.edges(src, range=(5, 6))       # range is not used with explicit edges
    assert np.array_equal(out, src) and out is not src
    assert H.edges(np.arange(H.MAX_BINS + 1)).size == H.MAX_BINS + 1


@pytest.mark.parametrize("bins", [0, -3, True, False, 2.5, 10.0, "10", None, [1.0], [], [[0, 1], [2, 3]],
                                  [0, 1, 1, 2], [0, 2, 1], [0, np.nan, 1], [0, 1, np.inf], [-np.inf, 0], ["a", "b"],
                                  H.MAX_BINS + 1, np.arange(H.MAX_BINS + 2)],
                         ids=repr)
def test_bad_bins(bins):
    with pytest.raises(ValueError):
        H.edges(bins, (0.0, 1.0))


@pytest.mark.parametrize("rng", [(0, np.inf), (-np.inf, 0), (np.nan, 1), (0, np.nan), (2, 1), (1,), (1, 2, 3), "ab",
                                 5, None, (0, "x")], ids=repr)
def test_bad_range(rng):
    with pytest.raises(ValueError):
        H.edges(10, rng)


def test_range_too_narrow_for_distinct_edges():
    with pytest.raises(ValueError):
        H.edges(1000, (1.0, np.nextafter(1.0, 2.0)))


# -- Active.histogram: what is refused before any device work ----------------------
def _var():
    return ChunkedVariable(name="v", shape=(4, 6), chunks=(2, 3), dtype=np.dtype("<f4"), chunk_index={}, attrs={},
                           filter_pipeline=None, reader=lambda off, size: b"")


@pytest.mark.parametrize("kw", [dict(bins=0), dict(bins=True), dict(bins=2.0), dict(bins=[1, 1, 2]), dict(bins=[3]),
                                dict(bins=4, range=(0, np.inf)), dict(bins=4, range=(np.nan, 1)),
                                dict(bins=4, range=(2, 1)), dict(bins=(1 << 20) + 1), dict(bins=(1 << 20) + 1, range=(0, 1)),
                                dict(bins=np.arange((1 << 20) + 2))], ids=repr)
def test_histogram_settings_raise_at_once(kw):
    with pytest.raises(ValueError):
        Active(_var()).histogram(**kw)


def test_histogram_sets_the_query_like_var_does():
    a = Active(_var())
    assert a.histogram(bins=4, range=(0, 1), axis=(1,)) is a
    assert a._method == "histogram" and a._axis == (1,)
    assert np.array_equal(a._hist["edges"], np.linspace(0, 1, 5)) and a._hist["uniform"]
    a.histogram([0, 1, 5])
    assert a._hist["n"] == 2 and not a._hist["uniform"]
    a.histogram()
    assert a._hist["n"] == 10 and a._hist["edges"] is None      # range=None: found by the query
    a.method = "mean"                                          # another method drops the bins
    assert a._hist is None


# -- bin_counts -----------------------------------------------------------------
def _numpy_counts(x, e):
    """np.histogram over explicit edges, plus below / above / nan by comparison."""
    fin = x[np.isfinite(x)]
    counts = np.histogram(fin, bins=e)[0].astype(np.int64)
    return counts, int((x < e[0]).sum()), int((x > e[-1]).sum()), int(np.isnan(x).sum())


def _planted(rng, e, n=2000):
    lo, hi = e[0], e[-1]
    span = hi - lo
    x = rng.uniform(lo - 0.2 * span, hi + 0.2 * span, n)
    plant = np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf)])
    x[rng.choice(n, plant.size, replace=False)] = plant
    return x


@pytest.mark.parametrize("seed", range(40))
def test_bin_counts_uniform_edges_match_np_histogram(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 200))
    lo = rng.normal(0, 10 ** rng.uniform(-3, 6))
    hi = lo + 10 ** rng.uniform(-3, 6)
    e = H.edges(n, (lo, hi))
    x = _planted(rng, e)
    got = H.bin_counts(x, e)
    want = _numpy_counts(x, e)
    assert got[0].dtype == np.int64 and np.array_equal(got[0], want[0])
    assert got[1:] == want[1:]
    # the range form of np.histogram bins the same way (it drops what lies outside)
    assert np.array_equal(got[0], np.histogram(x, bins=n, range=(lo, hi))[0])
    assert got[0].sum() + got[1] + got[2] + got[3] == x.size


@pytest.mark.parametrize("seed", range(20))
def test_bin_counts_explicit_edges_and_non_finite_values(seed):
    rng = np.random.default_rng(1000 + seed)
    e = np.unique(np.cumsum(rng.exponential(1.0, int(rng.integers(2, 60)))) - 10.0)
    x = _planted(rng, H.edges(e))
    x[rng.choice(x.size, 30, replace=False)] = np.repeat([np.nan, np.inf, -np.inf], 10)
    got = H.bin_counts(x.reshape(40, 50), e)
    want = _numpy_counts(x, e)
    assert np.array_equal(got[0], want[0]) and got[1:] == want[1:]
    assert got[3] == 10 and got[1] >= 10 and got[2] >= 10


def test_bin_counts_closed_last_bin_and_empty_input():
    e = np.array([0.0, 1.0, 2.0])
    c, below, above, nan = H.bin_counts([0.0, 1.0, 2.0, 2.0, np.nextafter(2.0, 3.0), -0.0, np.nextafter(0.0, -1.0)], e)
    assert c.tolist() == [2, 3] and (below, above, nan) == (1, 1, 0)
    c, below, above, nan = H.bin_counts(np.zeros(0), e)
    assert c.tolist() == [0, 0] and c.dtype == np.int64 and (below, above, nan) == (0, 0, 0)


# -- merge ------------------------------------------------------------------------
def test_merge_is_addition():
    rng = np.random.default_rng(5)
    e = H.edges(16, (-3, 3))
    x = rng.normal(0, 1.5, 5000)
    x[:5] = np.nan
    parts = [H.bin_counts(p, e) for p in (x[:1234], x[1234:])]
    whole = H.bin_counts(x, e)
    assert np.array_equal(H.merge(parts[0][0], parts[1][0]), whole[0])
    as_dict = lambda t: {"counts": t[0], "bin_edges": e, "n": np.int64(t[0].sum() + sum(t[1:])),
                         "below": np.int64(t[1]), "above": np.int64(t[2]), "nan": np.int64(t[3])}
    m = H.merge(as_dict(parts[0]), as_dict(parts[1]))
    w = as_dict(whole)
    assert set(m) == set(w)
    for k in w:
        assert np.array_equal(m[k], w[k]), k
    assert m["counts"].dtype == np.int64
    with pytest.raises(ValueError):
        H.merge(np.zeros(3, np.int64), np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        H.merge(as_dict(whole), dict(as_dict(whole), bin_edges=e + 1))
    with pytest.raises(ValueError):
        H.merge(as_dict(whole), whole[0])


# -- quantile -----------------------------------------------------------------------
def test_quantile_within_one_bin_width():
    rng = np.random.default_rng(11)
    x = rng.normal(288.0, 10.0, 100_000)
    e = H.edges(256, (x.min(), x.max()))
    counts = H.bin_counts(x, e)[0]
    q = np.array([0.0, 0.001, 0.01, 0.05, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 1.0])
    got = H.quantile(counts, e, q)
    width = e[1] - e[0]
    err = np.abs(got - np.quantile(x, q))
    print("quantile error / bin width", (err / width).max())
    assert got.shape == q.shape and (err <= width).all()
    assert abs(H.quantile(counts, e, 0.5) - np.median(x)) <= width
    # per output: (..., n_bins) -> (...,) + q.shape
    both = H.quantile(np.stack([counts, counts[::-1]]).reshape(2, 1, 256), e, q)
    assert both.shape == (2, 1, q.size) and np.array_equal(both[0, 0], got)
    assert np.isnan(H.quantile(np.zeros(256, np.int64), e, 0.5))
    with pytest.raises(ValueError):
        H.quantile(counts, e, 1.5)
    with pytest.raises(ValueError):
        H.quantile(counts[:-1], e, 0.5)
