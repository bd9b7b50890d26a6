"""The trend kernels' branches that ``tests/test_gpu_trend.py`` does not reach:
the T1, T2, C1, M and G6D cases of ``tests/_stats_gaps.py`` and its G2 to G5
cases, run through that module's own ``make_var``, ``oracle``, ``check`` and
``query``, so no tolerance is new.  ``tests/test_stats_gap_shapes.py`` checks
on the host that every shape reaches the branch it is named for.

Largest error over this file, measured on an MI355X: 4.93e-5 of the slope's
bound and of the intercept's, at the rank-8 case with two coordinate values
an output.
"""
import functools

import numpy as np
import pytest

from tests import _stats_gaps as G
from tests.test_gpu_trend import make_var, months, oracle, query, check, low_fill, trend, WORST

pytestmark = pytest.mark.gpu

MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


gap_var = functools.partial(G.variable, make_var)


def gap_check(group, name, dt, masked, run, shuffle=None):
    """One run of a case: the slope and, from the components, the intercept
    and n; the path the query took.  Returns the slope and the oracle."""
    iname, index, axis, along, path = run
    x, attrs, var = gap_var(group, name, dt, masked, shuffle)
    coord = months(x.shape[along])
    o = oracle(x, attrs, coord, along, index, axis)
    what = f"{group} {name} {dt} {'masked' if masked else 'plain'} {G.run_id(run)}"
    got, took = query(var, along, coord, axis, index)
    assert took == path, (what, took)
    check(got, o, what)
    comp, _ = query(var, along, coord, axis, index, components=True)
    np.testing.assert_array_equal(np.ma.getdata(comp["n"]), o["n"], err_msg=what)
    check(comp["intercept"], o, what, "intercept")
    return got, o


@MASKED
@pytest.mark.parametrize("name", list(G.T1))
def test_t1_reduced_positions_beyond_the_offset_map(low_fill, name, masked):
    """More than kTrendRoff reduced positions in a chunk: the radix-counter
    walk of k_trend_axes without a vector mask table, a wave ("row") and a
    lane ("lane") per output, with zero and non-zero starts; the coordinate
    along the outermost and along the innermost dim."""
    for run in G.runs("T1", name):
        gap_check("T1", name, "<f4", masked, run)


@MASKED
@pytest.mark.parametrize("dt", G.T_DTYPES["T2"], ids=lambda d: d.replace("|", "="))
@pytest.mark.parametrize("name", list(G.T2))
def test_t2_rows_beyond_one_staging_pass(low_fill, name, dt, masked):
    """More rows in a chunk layer than k_trend_cols stages per pass, and
    exactly as many; over two reduced dims the pass boundary falls inside a
    row of the second."""
    for run in G.runs("T2", name):
        assert run[4] == "cols"
        gap_check("T2", name, dt, masked, run)


@MASKED
@pytest.mark.parametrize("dt", G.T_DTYPES["C1"])
@pytest.mark.parametrize("name", list(G.C1))
def test_c1_several_workgroups_per_column(low_fill, name, dt, masked):
    """Columns of more than kBlock items: the second and third workgroup of
    k_trend_cols, idle lanes in the last, and the early return."""
    for run in G.runs("C1", name):
        assert run[4] == "cols"
        gap_check("C1", name, dt, masked, run)


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_second_trip_of_the_lane_loop(low_fill, name, masked):
    """16,900 kept outputs in a chunk, 16,384 lanes in k_trend_axes' launch;
    the same variable whole takes k_trend_cols with 17 workgroups a column."""
    k = G.G2_SECOND_TRIP
    paths = set()
    for run in G.runs("G2", name):
        got, o = gap_check("G2", name, "<f4", masked, run)
        assert got.shape == (1, 130, 130)
        tail = {key: v.reshape(-1)[k:] for key, v in o.items()}
        check(got.reshape(-1)[k:], tail, f"G2 {name} {run[0]}: the second trip, outputs {k}..16899")
        paths.add(run[4])
    assert paths == {"cols", "walk"}


@MASKED
@pytest.mark.parametrize("dt", G.G3_DTYPES)
@pytest.mark.parametrize("name", ["odd", "odd17"])
def test_g3_shuffled_chunks_of_odd_size(low_fill, name, dt, masked):
    """Shuffled chunks of 105 and 255 elements: no 4-element plane loads in
    k_trend_cols (whole and from row 1), byte planes at odd offsets in both
    kernels."""
    assert [run[4] for run in G.runs("G3", name)] == ["cols", "cols", "walk"]     # whole, from1, stride
    for run in G.runs("G3", name):
        gap_check("G3", name, dt, masked, run)


@MASKED
def test_g4_rank_8(low_fill, masked):
    for run in G.runs("G4", "8d"):
        gap_check("G4", "8d", "<f4", masked, run)
    assert {G.axis_id(r[2]) for r in G.runs("G4", "8d") if r[4] == "cols"} == {"0", "0123", "0123456"}


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(low_fill, dt, shuffle, masked):
    assert [run[4] for run in G.runs("G5", "dtypes")] == ["walk", "cols"]         # over (1,), over (0,)
    for run in G.runs("G5", "dtypes"):
        gap_check("G5", "dtypes", dt, masked, run, shuffle)


@pytest.mark.parametrize("mode", G.M_MODES)
@pytest.mark.parametrize("dt", G.M_DTYPES)
def test_mask_modes(low_fill, dt, mode):
    """Both equality rules with both thresholds, a lone missing_value and a
    lone valid_max, in k_trend_cols (whole) and k_trend_axes (strided)."""
    x, attrs, pad, _ = G.mask_case(dt, mode)
    var = make_var(x, G.M_CHUNKS, attrs, pad=pad)
    coord = months(x.shape[0])
    for (iname, index), path in zip(G.M_INDEXES.items(), ("cols", "walk")):
        got, took = query(var, 0, coord, (0,), index)
        assert took == path
        check(got, oracle(x, attrs, coord, 0, index, (0,)), f"M {dt} {mode} {iname}")


@pytest.mark.parametrize("dt,shuffle,off,vec", G.G6D_CASES, ids=G.G6D_IDS)
def test_g6_base_misaligned_under_the_column_kernel(gpu, dt, shuffle, off, vec):
    """One chunk ``off`` bytes into its buffer through pyas_trend_cols itself:
    the per-element fallback of the 4-element loads."""
    from pyactivestorage_amd import _lib, engine
    from pyactivestorage_amd.active import _grid_struct
    from pyactivestorage_amd.device import DeviceBuffer
    data = G.g6d_chunk(dt)
    assert (off % G.k_align(dt, shuffle) == 0) == vec
    coord = months(data.shape[0])
    st, buf, plan = G.misaligned_plan(gpu, data, off, shuffle=shuffle)
    n_out = int(np.prod(data.shape[1:]))
    cbuf, obuf = DeviceBuffer(gpu, coord.nbytes + 16), DeviceBuffer(gpu, n_out * _lib.COMOMENTS_NBYTES)
    gpu.h2d(cbuf.ptr, coord, st)
    gpu.h2d(cbuf.ptr + coord.nbytes, np.zeros(1, np.int32), st)
    grid = _grid_struct(3, (0,), (1,) + data.shape[1:], {"n_coords": [1, 1, 1]}, None, None)
    assert engine.trend_cols(gpu, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + coord.nbytes, 0, grid, obuf.ptr, st)
    rec = np.zeros(n_out, engine.comoments_dtype)
    gpu.d2h(rec, obuf.ptr, st)
    gpu.synchronize(st)
    rec = rec.reshape((1,) + data.shape[1:])
    o = oracle(data, None, coord, 0, Ellipsis, (0,))
    what = f"G6 {dt} {'shuffled' if shuffle else 'stored'} offset {off}"
    np.testing.assert_array_equal(rec["count"], o["n"], err_msg=what)
    check(trend.slope(rec), o, what)
    check(trend.intercept(rec), o, what, "intercept")


def setup_module(module):
    """This file's own maxima: test_gpu_trend's, in the shared WORST, are set aside."""
    module.BEFORE = dict(WORST)
    WORST.update(dict.fromkeys(WORST, 0.0))


def teardown_module(module):
    print("test_stats_gaps_trend: largest errors as fractions of the bounds:", WORST)
    WORST.update({k: max(v, BEFORE[k]) for k, v in WORST.items()})
