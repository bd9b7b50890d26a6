"""Host-side checks of the branch-coverage cases in ``tests/_stats_gaps.py``:
the shapes reach the branches they are named for, given the constants the
kernels are built with, and every case's data and reference are well-posed.
If a constant in ``csrc`` changes, this says which cases no longer reach
their branch."""
import os
import re

import numpy as np
import pytest

from pyactivestorage_amd import _lib
from tests import _stats_gaps as G

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "pyactivestorage_amd", "csrc")


def _text(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _const(name, text):
    m = re.search(rf"constexpr\s+int\s+{name}\s*=\s*(\d+)\s*;", text)
    assert m, f"{name} not found"
    return int(m.group(1))


K_BLOCK = _const("kBlock", _text("pyas_device.hpp"))
K_WAVE = _const("kWave", _text("pyas_device.hpp"))
K_MOM_ROFF = _const("kMomRoff", _text("pyas_moments.hip"))
K_COM_ROFF = _const("kComRoff", _text("pyas_comoments.hip"))


def test_launch_cap_is_the_launchers():
    """The five launchers still cap the workgroups per chunk at LAUNCH_CAP."""
    capi = _text("pyas_capi.hip")
    for fn in ("axes_geometry", "hist_axes_shape"):    # the two launch shapes
        start = re.search(rf"^(static )?(void|int64_t) {fn}\(", capi, re.M)
        assert start, fn
        body = capi[start.end():]
        body = body[:re.search(r"^}", body, re.M).start()]
        assert re.search(rf"if \(bpc > {G.LAUNCH_CAP}\) bpc = {G.LAUNCH_CAP};", body), fn
    for shape, fns in (("axes_geometry", ("pyas_moments_axes", "pyas_comoments_axes", "pyas_wsum_axes")),
                       ("hist_axes_shape", ("pyas_hist_axes", "pyas_select_axes"))):
        for fn in fns:
            start = re.search(rf"^int {fn}\(", capi, re.M)
            assert start, fn
            body = capi[start.end():]
            assert f"{shape}(" in body[:re.search(r"^}", body, re.M).start()], fn


def test_g1_reduced_positions_straddle_the_map():
    assert K_MOM_ROFF == K_COM_ROFF
    cap = K_MOM_ROFF

    def n_reds(name, iname):
        shape, chunks, axes, indexes, _ = G.case("G1", name)
        return sorted({r for r, _ in G.chunk_counts(shape, chunks, indexes[iname], axes[0])})

    for name in ("row", "lane"):
        lo, hi = n_reds(name, "whole")
        assert lo <= cap < hi and hi == cap + 1, (name, lo, hi)      # the map and the walk in one launch
        assert max(n_reds(name, "from")) <= cap                       # (this index is back under the map)
        assert hi > 4 * K_WAVE                                        # the wave form's unrolled loop runs
    assert n_reds("map", "whole") == [cap]
    for name in ("row-from", "lane-from"):                            # the walk with non-zero starts
        lo, hi = n_reds(name, "from")
        assert lo <= cap < hi, (name, lo, hi)
    # the wave form needs the innermost dim reduced, the lane form kept
    assert 2 in G.case("G1", "row")[2][0] and 2 not in G.case("G1", "lane")[2][0]


def test_g2_kept_outputs_exceed_one_trip():
    per_trip = G.LAUNCH_CAP * K_BLOCK
    assert G.G2_SECOND_TRIP == per_trip
    for name in G.G2:
        shape, chunks, axes, indexes, _ = G.case("G2", name)
        assert axes == [(0,)]                                          # innermost dim kept: a lane per output
        for n_red, n_keep in G.chunk_counts(shape, chunks, G.ALL, (0,)):
            assert per_trip < n_keep <= 2 * per_trip and n_red == 3, (name, n_keep)


def test_g3_shuffled_runs():
    for name, inner in (("odd", 7), ("odd17", 17)):
        shape, chunks, _, _, shuffled = G.case("G3", name)
        assert shuffled and int(np.prod(chunks)) % 16 != 0 and chunks[-1] == inner
        assert all(s % c for s, c in zip(shape, chunks))               # edge chunks in every dim
    assert G.case("G3", "odd17")[1][-1] >= 16                         # the weighted full kernel takes its runs
    shape, chunks, _, indexes, shuffled = G.case("G3", "runs")
    n = int(np.prod(chunks))
    assert shuffled and shape == chunks and n % 16 == 0 and chunks[-1] >= 16
    pos = np.arange(n).reshape(chunks)
    for iname, index in indexes.items():
        run = pos[index].reshape(-1)
        i0, i1 = G.G3_RUNS[iname]
        assert np.array_equal(run, np.arange(i0, i1)), iname           # one contiguous run
    g = lambda i0, i1: ((i0 + 15) & ~15, i1 & ~15)
    assert g(*G.G3_RUNS["80-320"]) == (80, 320)
    g0, g1 = g(*G.G3_RUNS["20-60"])
    assert 20 < g0 < g1 < 60                                           # head, groups and tail
    g0, g1 = g(*G.G3_RUNS["3-12"])
    assert g0 >= g1                                                    # shorter than a group


def test_g4_ranks():
    assert [len(G.case("G4", k)[0]) for k in ("1d", "2d", "4d", "8d")] == [1, 2, 4, _lib.MAX_DIMS]
    shape, chunks, axes, _, _ = G.case("G4", "8d")
    assert int(np.prod(shape)) == 3240 and int(np.prod([-(-s // c) for s, c in zip(shape, chunks)])) == 32
    assert sum(1 for s, c in zip(shape, chunks) if s % c) == 5


# -- the cases of the trend and grouped modules ---------------------------------------
ROOT = os.path.dirname(os.path.dirname(CSRC))
K_TREND_ROFF = _const("kTrendRoff", _text("pyas_trend.hip"))
K_TREND_ROWS = _const("kTrendRows", _text("pyas_internal.hpp"))
K_TREND_V = _const("kTrendV", _text("pyas_internal.hpp"))
K_GROUP_V = _const("kGroupV", _text("pyas_internal.hpp"))


def test_group_rows_is_the_headers():
    with open(os.path.join(ROOT, "include", "pyas.h")) as f:
        m = re.search(r"#define\s+PYAS_GROUP_ROWS\s+(\d+)", f.read())
    assert m and int(m.group(1)) == _lib.GROUP_ROWS
    assert re.search(r"constexpr\s+int\s+kGroupRows\s*=\s*PYAS_GROUP_ROWS\s*;", _text("pyas_internal.hpp"))


def test_dense_kernels_share_the_item_width_and_the_walks_the_launch_cap():
    """G.dense_columns restates the launchers' items and bpc (pyas_trend_cols,
    group_cols_run) from kTrendV / kGroupV and kBlock, read above; the C1 and
    T2 checks below hold one width for the three kernels."""
    capi = _text("pyas_capi.hip")
    assert K_TREND_V == K_GROUP_V
    for fn in ("pyas_trend_axes", "group_axes_run"):     # the walks' launches: LAUNCH_CAP workgroups a chunk
        start = re.search(rf"^(static )?int {fn}\(", capi, re.M)
        assert start, fn
        body = capi[start.end():]
        assert "axes_geometry(" in body[:re.search(r"^}", body, re.M).start()], fn


def test_t1_reduced_positions_straddle_the_trend_map():
    cap = K_TREND_ROFF

    def n_reds(name, iname):
        shape, chunks, axes, indexes, _ = G.case("T1", name)
        return sorted({r for r, _ in G.chunk_counts(shape, chunks, indexes[iname], axes[0])})

    for name, iname in (("row", "whole"), ("lane", "listed"), ("row-from", "from"), ("lane-from", "from")):
        lo, hi = n_reds(name, iname)
        assert lo <= cap < hi and hi == cap + 1, (name, lo, hi)      # the map and the walk in one launch
        assert hi > 4 * K_WAVE                                        # the wave form's unrolled loop runs
    assert n_reds("map", "whole") == [cap]
    for name in ("row-from", "lane-from"):                            # non-zero starts in the walking chunk
        index = G.index_of("T1", name, "from")
        assert index[0].start > 0 and max(ix.start or 0 for ix in index[1:] if isinstance(ix, slice)) > 0
    # the wave form needs the innermost dim reduced, the lane form kept; only the walk has the map
    for name in G.T1:
        row = 2 in G.case("T1", name)[2][0]
        assert row == (not name.startswith("lane"))
        walks = [r for r in G.runs("T1", name) if r[4] == "walk"]
        assert walks and all(r[0] != "whole" or row for r in walks), name
    assert {r[3] for r in G.runs("T1", "row")} == {0, 2}             # the coordinate along the innermost dim too


def test_t2_rows_per_layer_exceed_and_equal_one_pass():
    shape, chunks, axes, indexes, _ = G.case("T2", "rows")
    assert G.layer_rows(shape, chunks, indexes["whole"], axes[0]) == [(K_TREND_ROWS + 37, 0), (K_TREND_ROWS, 0)]
    assert G.layer_rows(shape, chunks, indexes["from37"], axes[0]) == [(K_TREND_ROWS, 37), (K_TREND_ROWS, 0)]
    shape, chunks, axes, indexes, _ = G.case("T2", "p2")
    rows = G.layer_rows(shape, chunks, indexes["whole"], axes[0])[0][0]
    assert axes == [(0, 1)] and K_TREND_ROWS < rows < 2 * K_TREND_ROWS
    assert K_TREND_ROWS % chunks[1]                                   # the pass boundary lies inside a row of dim 1
    assert {r[3] for r in G.runs("T2", "p2")} == {0, 1}
    # T1's lane case, whole, is dense too: two passes over two reduced dims
    shape, chunks, axes, indexes, _ = G.case("T1", "lane")
    assert G.layer_rows(shape, chunks, indexes["whole"], axes[0])[0][0] == 2 * K_TREND_ROWS + 1
    for name in G.T2:
        assert all(r[4] == "cols" for r in G.runs("T2", name))


def test_c1_columns_take_several_workgroups():
    for name, bpc in (("wg2", 2), ("wg3-4d", 3)):
        shape, chunks, axes, indexes, _ = G.case("C1", name)
        for iname, index in indexes.items():
            cols = G.dense_columns(shape, chunks, index, axes[0], K_TREND_V, K_BLOCK)
            assert {b for _, b in cols} == {bpc}, (name, iname)
            assert any(n > K_BLOCK for n, _ in cols), (name, iname)                       # a later workgroup works
            assert any(n > K_BLOCK and n % K_BLOCK for n, _ in cols), (name, iname)       # ... with idle lanes
            assert any(n <= (b - 1) * K_BLOCK for n, b in cols), (name, iname)            # the early return
        assert all(r[4] == "cols" for r in G.runs("C1", name))
    shape, chunks, axes, indexes, _ = G.case("C1", "wg2")
    whole = G.dense_columns(shape, chunks, indexes["whole"], axes[0], K_TREND_V, K_BLOCK)
    box = G.dense_columns(shape, chunks, indexes["box"], axes[0], K_TREND_V, K_BLOCK)
    assert whole[0][0] == 270 and box[0][0] == 240 and box[2][0] == 270   # a cut first column, dead lanes in its first workgroup
    shape, chunks, axes, _, _ = G.case("C1", "wg3-4d")
    assert len(shape) - 1 - len(axes[0]) == 1                        # a kept dim between the prefix and the innermost
    # the G2 variables, whole, are dense as well
    shape, chunks, _, _, _ = G.case("G2", "one")
    assert G.dense_columns(shape, chunks, G.ALL, (0,), K_TREND_V, K_BLOCK) == [(130 * 33, 17)]


def test_g2_walk_records_exceed_one_trip():
    per_trip = G.LAUNCH_CAP * K_BLOCK
    for name in G.G2:
        shape, chunks, _, _, _ = G.case("G2", name)
        walk = [r for r in G.runs("G2", name) if r[4] == "walk"]
        assert len(walk) == 1 and walk[0][2] == (0,) and walk[0][3] == 0
        for n_red, n_keep in G.chunk_counts(shape, chunks, walk[0][1], (0,)):
            assert n_red == 3 and per_trip < n_keep <= 2 * per_trip       # k_trend_axes: a second trip
            # k_group_axes under [0, 1, 0]: two local groups, three trips, group 1 wholly past the first
            assert 2 * per_trip < 2 * n_keep <= 3 * per_trip and n_keep >= G.G2_SECOND_TRIP


def _gap_runs():
    for group in ("T1", "T2", "C1", "G2", "G3", "G4", "G5"):
        for name in G.GROUPS[group]:
            if (group, name) == ("G3", "runs"):
                continue
            dts = {"G3": G.G3_DTYPES, "G5": G.G5_DTYPES, **G.T_DTYPES}.get(group, ["<f4"])
            for dt in dts:
                yield pytest.param(group, name, dt, id=f"{group}-{name}-{dt[1:]}{'be' if dt[0] == '>' else ''}")


# outputs of two elements: one masked element leaves no slope (NaN on both sides)
FEW_POINTS = {("G4", "8d", "strided", (0,))}


@pytest.mark.parametrize("group,name,dt", list(_gap_runs()))
def test_runs_are_well_posed(group, name, dt):
    """Every run of the trend and grouped modules: a masked case masks
    something but not everything, and every output keeps valid elements at
    two positions or more along the coordinate's dim."""
    nd = len(G.case(group, name)[0])
    for masked in (False, True):
        x, ax = G.single(group, name, dt, masked)
        m = np.ma.getmaskarray(G.masked_selection(x, ax, G.ALL))
        assert m.any() == masked and not m.all()
        for iname, index, axis, along, path in G.runs(group, name):
            assert along in (axis if axis is not None else range(nd))
            assert path == ("cols" if iname in ("whole", "from1", "from37", "box") and G.is_prefix(axis, nd) else "walk")
            sel = m[index]
            assert sel.any() == masked and not sel.all()
            points = G.trend_points(m, index, axis, along)
            assert points >= 2 or (masked and (group, name, iname, axis) in FEW_POINTS), (iname, axis, along, points)
        # the padding against the valid data (see G.pad_of): beyond them, but for G5's full-range integers
        valid = x[~m].astype(np.float64)
        pad = float(G.pad_of(dt))
        assert pad > valid.max() or (group == "G5" and np.dtype(dt).kind in "iu" and pad == valid.max()), (masked, pad)
        if not masked or np.dtype(dt).kind != "u":      # (an unsigned fill value is the padding itself)
            assert not np.ma.getmaskarray(G.masked_selection(np.array([G.pad_of(dt)], np.dtype(dt)), ax, G.ALL)).any()


@pytest.mark.parametrize("mode", G.M_MODES)
@pytest.mark.parametrize("dt", G.M_DTYPES)
def test_mask_cases_are_well_posed(dt, mode):
    from pyactivestorage_amd.variable import get_missing_attributes
    x, attrs, pad, plants = G.mask_case(dt, mode)
    fill, miss, lo, hi = get_missing_attributes(attrs)
    assert [v is not None for v in (fill, miss, lo, hi)] == {"both": [True] * 4, "missing": [False, True, False, False],
                                                            "max": [False, False, False, True]}[mode]
    if mode == "both":
        assert lo < fill < hi and lo < miss < hi                      # no rule is trimmed away
    m = np.ma.getmaskarray(G.masked_selection(x, attrs, G.ALL))
    for v, want in plants.items():
        hit = x == np.dtype(dt).type(v)
        assert hit.sum() >= 5 and (m[hit] == want).all(), (v, want)
    assert not np.ma.getmaskarray(G.masked_selection(np.array([pad]), attrs, G.ALL)).any()   # padding read would count
    assert mode != "missing" or pad > x.max()       # ... and without a valid_max it would be a max as well
    for index in G.M_INDEXES.values():
        index = G.per_dim(index, 3)
        assert m[index].any() and G.trend_points(m, index, (0,), 0) >= 2


def test_g6d_offsets_miss_and_keep_the_alignment():
    assert G.G6D_SHAPE[-1] % K_TREND_V == 0        # (so every byte plane of the shuffled chunk starts 4-aligned too)
    for dt, shuffled, off, vec in G.G6D_CASES:
        assert (off % G.k_align(dt, shuffled, K_TREND_V) == 0) == vec and 0 < off < 16
        assert shuffled or off % np.dtype(dt).itemsize == 0
    assert {(dt, sh) for dt, sh, _, vec in G.G6D_CASES if vec} == {("<f4", True)}


def _cases():
    for group, cases in G.GROUPS.items():
        for name in cases:
            dts = {"G3": G.G3_DTYPES, "G5": G.G5_DTYPES, **G.T_DTYPES}.get(group, ["<f4"])
            for dt in dts:
                yield pytest.param(group, name, dt, id=f"{group}-{name}-{dt[1:]}{'be' if dt[0] == '>' else ''}")


@pytest.mark.parametrize("group,name,dt", list(_cases()))
def test_cases_are_well_posed(group, name, dt):
    shape = G.case(group, name)[0]
    nat = np.dtype(dt).newbyteorder("=")
    for masked in (False, True):
        x, y, ax, ay = G.pair(group, name, dt, masked)
        assert x.shape == y.shape == shape and x.dtype == y.dtype == np.dtype(dt)
        assert bool(ax) == bool(ay) == masked
        if nat.kind == "i":
            assert x.min() < 0 < x.max()
            if masked:
                assert ax["_FillValue"][0] == np.iinfo(nat).min
        if nat == np.dtype(np.uint64):
            assert (x >= np.uint64(2 ** 63)).mean() >= 1 / 3 and (y >= np.uint64(2 ** 63)).mean() >= 1 / 3
            assert x.astype(np.float64).max() > 2.0 ** 63              # (never through int64)
            if masked:
                assert np.isin(np.array(G.U8_PLANTS, np.uint64), x).all()
                assert ax["valid_max"][0] == G.U8_MAX and ax["valid_min"][0] == G.U8_MIN
        r = float(np.corrcoef(x.astype(np.float64).ravel(), y.astype(np.float64).ravel())[0, 1])
        assert (0.2 < r < 0.8) or masked, r
        for iname, index, axis, need in G.combos(group, name):
            sx, sy = G.masked_selection(x, ax, index), G.masked_selection(y, ay, index)
            mx, my = np.ma.getmaskarray(sx), np.ma.getmaskarray(sy)
            both = mx | my
            if masked and (group, name) == ("G3", "runs"):      # (runs of 9 and 40 elements: run plain only)
                continue
            if masked:      # something is masked, not everything, and the two sides differ
                assert mx.any() and my.any() and not both.all() and (mx != my).any(), (iname, axis)
                assert not (mx & my).any()
            else:
                assert not both.any()
            valid = (~both).sum(axis=axis, keepdims=True)
            assert valid.min() >= max(need, 1), (iname, axis, int(valid.min()))
            if masked and need == 1:
                assert valid.min() == 1                                 # the case that says so
    if nat == np.dtype(np.uint64):
        x, _, ax, _ = G.pair(group, name, dt, True)
        m = np.ma.getmaskarray(G.masked_selection(x, ax, G.ALL))
        for v in G.U8_PLANTS:       # the integer comparison decides, not the float64 one
            want = v < G.U8_MIN or v > G.U8_MAX
            assert (m[x == np.uint64(v)] == want).all(), v
