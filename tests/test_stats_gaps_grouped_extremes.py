"""The grouped min / max / sum kernels' branches that
``tests/test_gpu_grouped_extremes.py`` does not reach: the C1, M and G6D cases
of ``tests/_stats_gaps.py`` and its G2 to G5 cases, run through that module's
own ``make_var``, ``oracle``, ``check`` and ``query``, so no tolerance is new.
``tests/test_stats_gap_shapes.py`` checks on the host that every shape reaches
the branch it is named for.
"""
import functools

import numpy as np
import pytest

from tests import _stats_gaps as G
from tests.test_gpu_grouped_extremes import make_var, oracle, query, check, cyclic, irregular, STATS, _lib, engine, grouped, WORST

pytestmark = pytest.mark.gpu

MASKED = pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])


gap_var = functools.partial(G.variable, make_var)


def gap_check(group, name, dt, masked, run, labels, n_g, shuffle=None, tail=None):
    """One run of a case under ``labels``: min, max and sum, and the path the
    queries took; ``tail``: the flat outputs from there on are checked on
    their own as well."""
    iname, index, axis, along, path = run
    x, attrs, var = gap_var(group, name, dt, masked, shuffle)
    o = oracle(x, attrs, labels, along, index, axis, n_g)
    what = f"{group} {name} {dt} {'masked' if masked else 'plain'} {G.run_id(run)}"
    for stat in STATS:
        got, took = query(var, stat, along, labels, axis, index, 0, n_g)
        assert took == path, (what, took)
        check(got, o, stat, dt, f"{what} {stat}")
        if tail is not None:
            check(got.reshape(-1)[tail:], {key: v.reshape(-1)[tail:] for key, v in o.items()}, stat, dt,
                  f"{what} {stat}: records {tail} on")


@MASKED
@pytest.mark.parametrize("dt", G.T_DTYPES["C1"])
@pytest.mark.parametrize("name", list(G.C1))
def test_c1_several_workgroups_per_column(gpu, name, dt, masked):
    """Columns of more than kBlock items: the second and third workgroup of
    k_group_cols_partial, idle lanes in the last, and the early return.  The
    padding is beyond every datum: read, it would be a max."""
    for run in G.runs("C1", name):
        assert run[4] == "cols"
        for pattern in (cyclic, irregular):
            gap_check("C1", name, dt, masked, run, *pattern(G.case("C1", name)[0][run[3]]))


@MASKED
@pytest.mark.parametrize("name", list(G.G2))
def test_g2_later_trips_of_the_lane_loop(gpu, name, masked):
    """Two local groups of 16,900 kept outputs in a chunk, 16,384 lanes in
    k_group_axes_partial's launch: three trips, every record of the second
    group past the first; the same variable whole takes k_group_cols_partial
    with 17 workgroups a column."""
    labels = np.resize([0, 1, 0], G.case("G2", name)[0][0])
    paths = set()
    for run in G.runs("G2", name):
        gap_check("G2", name, "<f4", masked, run, labels, 2, tail=G.G2_SECOND_TRIP)
        paths.add(run[4])
    assert paths == {"cols", "walk"}


@MASKED
@pytest.mark.parametrize("dt", G.G3_DTYPES)
@pytest.mark.parametrize("name", ["odd", "odd17"])
def test_g3_shuffled_chunks_of_odd_size(gpu, name, dt, masked):
    """Shuffled chunks of 105 and 255 elements: no 4-element plane loads in
    k_group_cols_partial (whole and from row 1), byte planes at odd offsets in
    both kernels."""
    assert [run[4] for run in G.runs("G3", name)] == ["cols", "cols", "walk"]     # whole, from1, stride
    for k, run in enumerate(G.runs("G3", name)):
        gap_check("G3", name, dt, masked, run, *(cyclic, irregular)[k % 2](G.case("G3", name)[0][run[3]]))


@MASKED
@pytest.mark.parametrize("name", list(G.G4))
def test_g4_ranks(gpu, name, masked):
    shape = G.case("G4", name)[0]
    for k, run in enumerate(G.runs("G4", name)):
        gap_check("G4", name, "<f4", masked, run, *(cyclic, irregular)[k % 2](shape[run[3]]))
    dense = {G.axis_id(r[2]) for r in G.runs("G4", name) if r[4] == "cols"}
    assert dense == {"1d": set(), "2d": {"0"}, "4d": {"0"}, "8d": {"0", "0123", "0123456"}}[name]


@MASKED
@pytest.mark.parametrize("dt,shuffle", G.G5_LAYOUTS, ids=lambda v: {False: "plain", True: "shuffled"}.get(v, v))
def test_g5_dtypes(gpu, dt, shuffle, masked):
    assert [run[4] for run in G.runs("G5", "dtypes")] == ["walk", "cols"]         # over (1,), over (0,)
    for run in G.runs("G5", "dtypes"):
        gap_check("G5", "dtypes", dt, masked, run, *cyclic(G.case("G5", "dtypes")[0][run[3]]), shuffle=shuffle)


@pytest.mark.parametrize("mode", G.M_MODES)
@pytest.mark.parametrize("dt", G.M_DTYPES)
def test_mask_modes(gpu, dt, mode):
    """Both equality rules with both thresholds, a lone missing_value and a
    lone valid_max, in k_group_cols_partial (whole) and k_group_axes_partial
    (strided)."""
    x, attrs, pad, _ = G.mask_case(dt, mode)
    var = make_var(x, G.M_CHUNKS, attrs, pad=pad)
    labels, n_g = cyclic(x.shape[0])
    for (iname, index), path in zip(G.M_INDEXES.items(), ("cols", "walk")):
        o = oracle(x, attrs, labels, 0, index, (0,), n_g)
        for stat in STATS:
            got, took = query(var, stat, 0, labels, (0,), index, 0, n_g)
            assert took == path
            check(got, o, stat, dt, f"M {dt} {mode} {iname} {stat}")


@pytest.mark.parametrize("dt,shuffle,off,vec", G.G6D_CASES, ids=G.G6D_IDS)
def test_g6_base_misaligned_under_the_column_kernel(gpu, dt, shuffle, off, vec):
    """One chunk ``off`` bytes into its buffer through pyas_group_cols_partial
    itself: the per-element fallback of the 4-element loads."""
    from pyactivestorage_amd.active import _grid_struct
    from pyactivestorage_amd.device import DeviceBuffer
    from pyactivestorage_amd.indexing import OrthogonalIndexer
    data = G.g6d_chunk(dt)
    assert (off % G.k_align(dt, shuffle) == 0) == vec
    labels, n_g = G.G6D_LABELS, 3
    dims = [list(d) for d in OrthogonalIndexer((Ellipsis,), data.shape, data.shape).dim_indexers]
    rows = grouped.row_list(dims[:1], data.shape, labels, 0, n_g)
    blob = np.concatenate([rows.layer, rows.offset, rows.label, np.zeros(1, dtype=np.int32)])
    st, buf, plan = G.misaligned_plan(gpu, data, off, shuffle=shuffle)
    n_out = int(np.prod(data.shape[1:]))
    rbuf, obuf = DeviceBuffer(gpu, blob.nbytes), DeviceBuffer(gpu, n_g * n_out * _lib.PARTIAL_NBYTES)
    gpu.h2d(rbuf.ptr, blob, st)
    grid = _grid_struct(3, (0,), (1,) + data.shape[1:], {"n_coords": [1, 1, 1]}, None, None)
    assert engine.group_cols(gpu, plan.batch, plan.mask_up.struct, rbuf.ptr, rbuf.ptr + 4 * rows.n_rows,
                             rbuf.ptr + 8 * rows.n_rows, rows.n_rows, n_g, grid, obuf.ptr, st, partial=True)
    rec = np.zeros(n_g * n_out, engine.partial_dtype(data.dtype))
    gpu.d2h(rec, obuf.ptr, st)
    gpu.synchronize(st)
    rec = rec.reshape((n_g,) + data.shape[1:])
    o = oracle(data, None, labels, 0, Ellipsis, (0,), n_g)
    what = f"G6 {dt} {'shuffled' if shuffle else 'stored'} offset {off}"
    np.testing.assert_array_equal(rec["count"], o["n"], err_msg=what)
    for stat in STATS:
        check(grouped.finalize(rec, stat, dtype=data.dtype), o, stat, dt, f"{what} {stat}")


def setup_module(module):
    """This file's own maxima: test_gpu_grouped_extremes's, in the shared WORST, are set aside."""
    module.BEFORE = dict(WORST)
    WORST.update(dict.fromkeys(WORST, 0.0))


def teardown_module(module):
    print("test_stats_gaps_grouped_extremes: largest float-sum error as a fraction of its bound:", WORST)
    WORST.update({k: max(v, BEFORE[k]) for k, v in WORST.items()})
