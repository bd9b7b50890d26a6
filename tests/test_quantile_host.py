"""The host side of ``Active.quantile`` (``pyactivestorage_amd.quantile``):
keys and their inverse, the NumPy statement of the radix select, ranks and
interpolation against ``np.quantile``, and the argument refusals of the public
interface.  Every comparison is exact; no device is needed.
"""
import numpy as np
import pytest

from pyactivestorage_amd import histogram as H
from pyactivestorage_amd import quantile as Q
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.variable import ChunkedVariable

# the ten dtypes of PYAS_HIST_DISPATCH
DTYPES = ["i1", "u1", "i2", "u2", "i4", "u4", "i8", "u8", "f4", "f8"]


def sample(dt, n=600, seed=0):
    """Values of ``dt`` with its extremes and hard cases: +-inf, +-0.0,
    denormals, int64 beyond +-2^53, uint64 above 2^63, and ties."""
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed + DTYPES.index(dt.str[1:]))
    if dt.kind == "f":
        fi = np.finfo(dt)
        x = rng.normal(0.0, 50.0, n).astype(dt)
        hard = [np.inf, -np.inf, 0.0, -0.0, fi.max, -fi.max, fi.tiny, -fi.tiny, fi.smallest_subnormal,
                -fi.smallest_subnormal, fi.tiny / 4, 1.0, np.nextafter(dt.type(1.0), dt.type(2.0)), -1.0]
        x[:len(hard)] = np.array(hard, dtype=dt)
    else:
        ii = np.iinfo(dt)
        x = rng.integers(ii.min, ii.max, n, dtype=dt, endpoint=True)
        hard = [ii.min, ii.max, 0, 1, ii.max - 1, ii.min + 1]
        if dt == np.dtype("i8"):
            hard += [2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2, -(2 ** 53), -(2 ** 53) - 1, -(2 ** 53) - 2]
        if dt == np.dtype("u8"):
            hard += [2 ** 63 - 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2]
        x[:len(hard)] = np.array(hard, dtype=dt)
    x[-20:] = x[:20]      # ties
    return x


@pytest.mark.parametrize("dt", DTYPES)
def test_keys_preserve_order_and_invert(dt):
    x = sample(dt)
    k = Q.keys(x)
    assert k.dtype == (np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32) and k.shape == x.shape
    assert Q.key_width(dt) == k.dtype.itemsize * 8
    # strictly order-preserving: keys compare exactly as the values do
    i, j = np.meshgrid(np.arange(x.size), np.arange(x.size), indexing="ij")
    assert np.array_equal(k[i] < k[j], x[i] < x[j])
    assert np.array_equal(k[i] == k[j], x[i] == x[j])
    back = Q.values(k, dt)
    assert back.dtype == np.dtype(dt) and np.array_equal(back, x)      # == : -0.0 comes back as +0.0
    if np.dtype(dt).kind == "f":
        z = np.array([0.0, -0.0], dtype=dt)
        assert Q.keys(z)[0] == Q.keys(z)[1]
        assert not np.signbit(Q.values(Q.keys(z), dt)).any()
    # the stored byte order does not matter
    assert np.array_equal(Q.keys(x.astype(np.dtype(dt).newbyteorder(">"))), k)


@pytest.mark.parametrize("bits", [1, 3, 8, 11])
@pytest.mark.parametrize("dt", DTYPES)
def test_select_is_the_sorted_element(dt, bits):
    x = sample(dt, n=300)
    k = Q.keys(x)
    width = k.dtype.itemsize * 8
    want = np.sort(x)
    for r in (0, 1, 149, 150, 298, 299):
        key, tables = Q.select(k, r, bits)
        assert Q.values(key, dt) == want[r], (dt, bits, r)
        assert len(tables) == -(-width // bits)                     # exactly ceil(width / bits) passes
        for (shift, b), row in zip(Q.digits(width, bits), tables):
            assert row.dtype == np.int64 and row.size == (1 << b) + 3
            assert row.sum() == x.size and row[-1] == 0             # counts + below + above + nan == n
        assert tables[0][-3] == 0 and tables[0][-2] == 0            # nothing lies above the first digit


def test_digits_cover_the_key():
    assert Q.digits(32, 11) == [(21, 11), (10, 11), (0, 10)]
    assert Q.digits(64, 8) == [(56 - 8 * i, 8) for i in range(8)]
    for width in (32, 64):
        for bits in range(1, Q.MAX_BITS + 1):
            d = Q.digits(width, bits)
            assert sum(b for _, b in d) == width and d[-1][0] == 0 and len(d) == -(-width // bits)
    for bad in (0, Q.MAX_BITS + 1):
        with pytest.raises(ValueError):
            Q.digits(32, bad)


def test_fit_bits_narrows_to_the_cap():
    assert Q.fit_bits(1, H.TABLE_CAP_BYTES) == Q.DIGIT_BITS
    assert Q.fit_bits(10, 10 * (8 + 3) * 8, want=8) == 3
    assert Q.fit_bits(10, 10 * 5 * 8, want=8) == 1
    with pytest.raises(ValueError, match=r"400 bytes.*399 bytes"):
        Q.fit_bits(10, 399, want=8)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


@pytest.mark.parametrize("method", Q.METHODS)
def test_ranks_and_finalize_equal_numpy(method):
    rng = np.random.default_rng(5)
    qs = np.concatenate([[0.0, 1.0, 0.5, 0.25, 0.95, 1.0 / 3.0], rng.random(40)])
    for n in (1, 2, 3, 1000, 4097):
        x = np.sort(rng.normal(0.0, 1e3, n))
        x[rng.integers(0, n, n // 10)] = 7.0      # ties
        x.sort()
        h, lo, hi = Q.ranks(n, qs, method)
        assert lo.dtype == np.int64 and lo.min() >= 0 and hi.max() <= n - 1 and np.all(lo <= hi)
        if method in ("lower", "higher", "nearest"):
            assert np.array_equal(lo, hi)
        got = Q.finalize(x[lo], x[hi], h, method)
        want = np.quantile(x, qs, method=method)
        assert got.dtype == np.float64 and np.array_equal(got, want), (method, n)
        # per-row n broadcasts against q
        h2, lo2, hi2 = Q.ranks(np.array([n, 1])[:, None], qs[None, :], method)
        assert np.array_equal(lo2[0], lo) and np.array_equal(hi2[0], hi) and not lo2[1].any()


def test_finalize_with_infinities_is_numpys():
    x = np.array([-np.inf, -np.inf, -1.0, 2.0, 5.0, np.inf, np.inf])
    qs = np.array([0.0, 0.1, 0.2, 0.4, 0.5, 0.9, 1.0])
    for method in Q.METHODS:
        h, lo, hi = Q.ranks(x.size, qs, method)
        with np.errstate(invalid="ignore"):
            want = np.quantile(x, qs, method=method)
        assert same(Q.finalize(x[lo], x[hi], h, method), want), method


def test_empty_rows_have_rank_zero():
    h, lo, hi = Q.ranks(np.array([0, 0, 5])[:, None], np.array([0.0, 0.5, 1.0])[None, :], "linear")
    assert not lo[:2].any() and not hi[:2].any() and list(lo[2]) == [0, 2, 4]


# -- the public interface: refusals before any device work ---------------------------
def in_memory():
    data = np.arange(24, dtype="<f4").reshape(4, 6)
    blob = data.tobytes()
    return ChunkedVariable(name="v", shape=data.shape, chunks=data.shape, dtype=data.dtype,
                           chunk_index={(0, 0): (0, len(blob))}, attrs={}, filter_pipeline=None,
                           reader=lambda off, size: blob[off:off + size])


@pytest.mark.parametrize("q", [-0.1, 1.5, float("nan"), [0.2, 1.01], [[0.1, 0.2]], "half", None])
def test_bad_q_is_refused(q):
    with pytest.raises(ValueError):
        Active(in_memory()).quantile(q)


def test_bad_method_is_refused():
    with pytest.raises(ValueError, match="method"):
        Active(in_memory()).quantile(0.5, method="hazen")


def test_weights_are_refused():
    a = Active(in_memory())
    a.weights = {0: np.ones(4)}
    a.quantile(0.5)
    with pytest.raises(ValueError, match="weights"):
        a[...]
    with pytest.raises(TypeError):
        Active(in_memory()).quantile(0.5, weights={0: np.ones(4)})


def test_group_is_refused():
    a = Active(in_memory(), group=object())
    a.median()
    with pytest.raises(NotImplementedError, match="quantile"):
        a[...]


def test_integer_index_is_refused():
    a = Active(in_memory())
    a.quantile([0.1, 0.9], axis=(1,))
    with pytest.raises(IndexError):
        a[2, :]


def test_table_beyond_the_cap_is_refused(monkeypatch):
    monkeypatch.setattr(H, "TABLE_CAP_BYTES", 6 * 5 * 8 - 1)     # 6 outputs of 1-bit digits take 240 bytes
    a = Active(in_memory())
    a.quantile(0.5, axis=(0,))
    with pytest.raises(ValueError, match=r"240 bytes.*239 bytes"):
        a[...]


def test_settings_hold_for_one_query():
    a = Active(in_memory())
    a.quantile([0.25, 0.75], axis=(0,), method="lower")
    assert a._method == "quantile" and a._quant["method"] == "lower" and list(a._quant["q"]) == [0.25, 0.75]
    with pytest.raises(IndexError):
        a[0, :]
    assert a._method is None and a._quant is None
    a.median()
    assert a._quant["q"].shape == () and float(a._quant["q"]) == 0.5 and a._quant["method"] == "linear"
    a.method = "mean"
    assert a._quant is None
