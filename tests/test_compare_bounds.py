"""``tests/_compare.sum_bound`` must bite: every legitimate summation order
stays inside it and every float32 temporary on a float64 path falls outside
it, at the sizes the GPU accuracy tests reduce per output (n <= 1024; the
worst-case bound grows as n * sum|x|, so beyond that a single narrowed
element hides in it).

Conditions, not measurements: zero legitimate rejections and zero missed
faults over every seeded draw.  The data are uniform draws that carry full
mantissas (a float32-representable value would make a narrowing invisible).
"""
import numpy as np
import pytest

from tests import _compare as C

SIZES = [2, 4, 7, 35, 210, 1024]
DRAWS = 60


def _draw(n, seed, dtype):
    rng = np.random.default_rng(1000 * n + seed)
    x = rng.uniform(-50, 150, size=n)
    if dtype == np.float32:
        x = x.astype(np.float32)
    else:                                   # no element is float32-representable
        assert (x.astype(np.float32).astype(np.float64) != x).all()
    return rng, x


def _seq(x):
    return float(np.cumsum(np.asarray(x, dtype=np.float64))[-1])      # cumsum adds left to right


def _tree(x, rng):
    """A random binary tree of f64 additions."""
    x = [float(v) for v in x]
    while len(x) > 1:
        i = int(rng.integers(0, len(x) - 1))
        x[i:i + 2] = [x[i] + x[i + 1]]
    return x[0]


def _groups_f32(x, gs, rng):
    """Groups of ``gs`` consecutive values added in float32 from a float32
    zero (TileAcc::add_group), the group sums in a random f64 tree."""
    parts = []
    for k in range(0, len(x), gs):
        g = np.float32(0)
        for v in x[k:k + gs]:
            g = np.float32(g + np.float32(v))
        parts.append(float(g))
    return _tree(parts, rng)


def _ref(x):
    ex = C.exact_reference(np.asarray(x, dtype=np.float64))
    return float(ex["exact"][0]), float(ex["abs_sum"][0]), int(ex["n"][0])


def _inside(got, want, bound):
    return bool(C.error_ratio(got, want, bound) <= 1.0)


@pytest.mark.parametrize("n", SIZES)
def test_f64_orders_pass_and_f32_temporaries_fail(n):
    worst = 0.0
    for seed in range(DRAWS):
        rng, x = _draw(n, seed, np.float64)
        exact, s, cnt = _ref(x)
        assert cnt == n
        b = float(C.sum_bound(np.float64, n, s, "sum"))
        b_np = float(C.sum_bound(np.float64, n, s, "sum", ref="numpy"))
        assert 0 < b < b_np
        for name, got in (("np.sum", float(np.sum(x))), ("sequential", _seq(x)), ("reversed", _seq(x[::-1])),
                          ("shuffled", _seq(rng.permutation(x))), ("tree", _tree(x, rng))):
            assert _inside(got, exact, b), (name, n, seed, got, exact, b)
            assert _inside(got, float(np.sum(x)), b_np), (name, "vs numpy", n, seed)
            worst = max(worst, float(C.error_ratio(got, exact, b)))
        # one element through float32
        y = x.copy()
        k = int(rng.integers(0, n))
        y[k] = np.float32(y[k])
        for got in (float(np.sum(y)), _seq(y)):
            assert not _inside(got, exact, b), ("element", n, seed, k, x[k], got, exact, b)
            if n <= 210:      # the doubled bound against NumPy's own sum hides some at 1024
                assert not _inside(got, float(np.sum(x)), b_np), ("element vs numpy", n, seed, k)
        # one partial (a quarter of the elements, at least one) through float32
        q = max(1, n // 4)
        got = float(np.float32(np.sum(x[:q]))) + float(np.sum(x[q:]))
        assert not _inside(got, exact, b), ("partial", n, seed, got, exact, b)
        # the final sum through float32
        got = float(np.float32(np.sum(x)))
        assert not _inside(got, exact, b), ("final", n, seed, got, exact, b)
        # the mean: one f64 division passes, a float32 division does not
        mean = exact / n
        bm = float(C.sum_bound(np.float64, n, s, "mean", mean_abs=mean))
        assert _inside(float(np.sum(x)) / n, mean, bm), ("mean", n, seed)
        assert _inside(float(np.mean(x)), mean, bm), ("np.mean", n, seed)
        got = float(np.float32(np.sum(x)) / np.float32(n))
        assert not _inside(got, mean, bm), ("mean in f32", n, seed, got, mean, bm)
        got = float(np.float32(np.sum(x) / n))
        assert not _inside(got, mean, bm), ("mean rounded to f32", n, seed, got, mean, bm)
    assert worst < 1.0


@pytest.mark.parametrize("n", SIZES)
def test_f32_groups_of_four_pass_and_f32_temporaries_fail(n):
    for seed in range(DRAWS):
        rng, x = _draw(n, seed, np.float32)
        exact, s, cnt = _ref(x)
        b = float(C.sum_bound(np.float32, n, s, "sum"))
        for gs in (1, 2, 4):
            got = _groups_f32(x, gs, rng)
            assert _inside(got, exact, b), ("groups", gs, n, seed, got, exact, b)
        assert _inside(_seq(x), exact, b) and _inside(_tree(x, rng), exact, b), (n, seed)
        # (one more float32 rounding of |sum| <= sum|x| is a fourth of the
        # gamma_3 term: this bound cannot see it; the sixteen-group case can)


def _ramp_groups(m, rng):
    """m groups of 16 float32 values [big, 14 x small, -big]: big in [1, 1.5),
    each small between 0.5 and 0.625 of big's ulp, so every float32 addition
    onto the running sum rounds up by at least 0.375 ulp: a 16-group in f32
    is off by >= 14 * 0.75 u32 > gamma_3 * sum|x| ~ 6 u32, while groups of
    four lose at most 3 + 1 roundings of u32 * big."""
    out = []
    for _ in range(m):
        big = np.float32(rng.uniform(1.0, 1.5))
        small = (rng.uniform(0.5, 0.625, size=14) * 2.0 ** -23).astype(np.float32)
        out.append(np.concatenate([[big], small, [-big]]).astype(np.float32))
    return np.concatenate(out)


@pytest.mark.parametrize("m", [1, 4, 64])
def test_f32_groups_of_sixteen_fail_where_four_pass(m):
    for seed in range(DRAWS):
        rng = np.random.default_rng(77 * m + seed)
        x = _ramp_groups(m, rng)
        exact, s, n = _ref(x)
        b = float(C.sum_bound(np.float32, n, s, "sum"))
        assert _inside(_groups_f32(x, 4, rng), exact, b), ("four", m, seed)
        got = _groups_f32(x, 16, rng)
        assert not _inside(got, exact, b), ("sixteen", m, seed, got, exact, b)


def test_non_finite_and_empty_outputs_get_no_tolerance():
    for s in (np.inf, np.nan):
        assert C.sum_bound(np.float64, 8, s) == 0.0
        assert C.sum_bound(np.float32, 8, s, "mean") == 0.0
    assert C.sum_bound(np.float64, 0, 0.0) == 0.0
    assert C.error_ratio(np.nan, np.nan, 0.0) == 0.0 and C.error_ratio(np.inf, np.inf, 0.0) == 0.0
    assert C.error_ratio(1.0, np.nan, 0.0) == np.inf and C.error_ratio(np.inf, -np.inf, 0.0) == np.inf
    with pytest.raises(AssertionError):
        C.assert_within(np.array([1.0]), np.array([np.inf]), C.sum_bound(np.float64, 3, np.inf))
    v = np.ma.MaskedArray(np.array([[1.5, np.nan, 2.0], [0.1, 0.2, 0.3], [9.0, 9.0, 9.0]]),
                          mask=[[0, 0, 0], [0, 1, 0], [1, 1, 1]])
    ex = C.exact_reference(v, (1,))
    assert np.isnan(ex["exact"][0]) and not np.isfinite(ex["abs_sum"][0])
    assert ex["exact"][1] == 0.1 + 0.3 and list(ex["n"]) == [3, 2, 0] and ex["exact"][2] == 0.0
    if np.finfo(np.longdouble).nmant >= 63:
        exl = C.exact_reference(v, (1,), extended=True)
        assert exl["exact"][1] == ex["exact"][1]


def test_assert_same_refuses_an_f64_sum_without_its_scale():
    w = np.ma.MaskedArray(np.array([[3.25]]))
    with pytest.raises(TypeError):
        C.assert_same(w, w.copy(), "sum")
    with pytest.raises(TypeError):
        C.assert_same(w, w.copy(), "mean", np.array([[3.25]]))
    with pytest.raises(TypeError):
        C.assert_same(w, w.copy(), "mean", np.array([[3.25]]), n=np.array([[1]]))
    with pytest.raises(TypeError):
        C.assert_same(w, w.copy(), "mean", data_dtype="<i4")
    C.assert_same(w, w.copy(), "sum", np.array([[3.25]]), n=np.array([[1]]), data_dtype="<f8")
    C.assert_same(w, w.copy(), "mean", data_dtype="<f4")      # an f64 mean of f32 data: the float32 rule
    C.assert_same(w, w.copy(), "max")
    w32 = w.astype(np.float32)
    C.assert_same(w32, w32.copy(), "sum")                     # float32 keeps REL_TOL
    # 3e-8 relative (one float32 rounding) is inside 1e-6 and outside the f64 bound
    x = np.random.default_rng(5).uniform(-50, 150, size=35)
    s, a = np.ma.MaskedArray(np.array([x.sum()])), np.array([np.abs(x).sum()])
    bad = np.ma.MaskedArray(np.array([float(np.float32(x.sum()))]))
    assert abs(bad[0] - s[0]) < C.REL_TOL * abs(s[0])
    with pytest.raises(AssertionError):
        C.assert_same(s, bad, "sum", a, n=np.array([35]), data_dtype=">f8")
    C.assert_same(s, bad, "sum", a, n=np.array([35]), data_dtype="<f4")
    with pytest.raises(AssertionError):
        C.assert_same(s / 35, np.ma.MaskedArray(np.array([float(np.float32(x.sum()) / np.float32(35))])),
                      "mean", a, n=np.array([35]), data_dtype="<i8")
