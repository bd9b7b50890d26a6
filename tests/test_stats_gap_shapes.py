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


def _cases():
    for group, cases in G.GROUPS.items():
        for name in cases:
            dts = {"G3": G.G3_DTYPES, "G5": G.G5_DTYPES}.get(group, ["<f4"])
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
