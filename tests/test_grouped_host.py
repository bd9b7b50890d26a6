"""Host side of ``Active.grouped``: the label checks, the sorted row list of
the dense path, the per-chunk group lists and segments of the walk path (both
replayed in NumPy against a direct per-group selection), ``grouped.finalize``
and the ``Active`` argument checks that run before any device call."""
import ctypes
import itertools

import numpy as np
import pytest

from pyactivestorage_amd import _lib, engine, grouped, moments
from pyactivestorage_amd.active import Active
from pyactivestorage_amd.indexing import OrthogonalIndexer
from pyactivestorage_amd.variable import ChunkedVariable


def _var(shape=(2, 3, 4)):
    data = np.arange(int(np.prod(shape)), dtype="<f4").reshape(shape)
    raw = data.tobytes()
    return ChunkedVariable(name="v", shape=data.shape, chunks=data.shape, dtype=np.dtype("<f4"),
                           chunk_index={(0,) * len(shape): (0, len(raw))}, reader=lambda off, size: raw[off:off + size])


# -- bindings -------------------------------------------------------------------
def test_bindings():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("pyas_group_cols", "pyas_group_axes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES
    assert _lib.GROUP_ROWS == 1024
    assert ctypes.sizeof(_lib.GroupRows) == 40 and ctypes.sizeof(_lib.GroupLists) == 32
    with open(_lib.LIB_DIR + "/../../include/pyas.h") as f:
        assert f"#define PYAS_GROUP_ROWS {_lib.GROUP_ROWS} " in f.read()


# -- check_labels ---------------------------------------------------------------
def test_check_labels_accepts():
    lab, g = grouped.check_labels([0, 2, -1, 2], 4)
    assert lab.dtype == np.int64 and lab.tolist() == [0, 2, -1, 2] and g == 3
    assert grouped.check_labels(np.array([1, 0], dtype=np.uint8), 2)[1] == 2
    assert grouped.check_labels(np.array([-5, -1], dtype=np.int16), 2)[1] == 0      # every label negative
    assert grouped.check_labels([0, 1], 2, n_groups=5)[1] == 5                      # more groups than labels need
    assert grouped.check_labels([-1, -1], 2, n_groups=0)[1] == 0
    assert grouped.check_labels(np.zeros(0, dtype=np.int64), 0) [1] == 0
    assert grouped.check_labels([3], 1, n_groups=np.int64(4))[1] == 4


@pytest.mark.parametrize("labels,n,n_groups", [
    ([0.0, 1.0], 2, None),                   # floats
    ([True, False], 2, None),                # bools
    ([0, 1, 2], 2, None),                    # a wrong length
    ([[0, 1]], 2, None),                     # not 1-D
    ([0, 3], 2, 3),                          # a label >= n_groups
    ([0, 1], 2, -1),
    ([0, 1], 2, 2.0),
    ([0, 1], 2, True),
    (["a", "b"], 2, None),
    ([0, 2 ** 31], 2, None),
])
def test_check_labels_rejects(labels, n, n_groups):
    with pytest.raises(ValueError):
        grouped.check_labels(labels, n, n_groups)


# -- the dense path's row list ---------------------------------------------------
SHAPE, CHUNKS = (15, 22, 37), (8, 12, 20)


def _rows(index, labels, along, P, n_groups):
    ix = OrthogonalIndexer(index, SHAPE, CHUNKS)
    dims = [list(d) for d in ix.dim_indexers]
    return dims, grouped.row_list(dims[:P], CHUNKS, np.asarray(labels, dtype=np.int64), along, n_groups)


def _global_rows(dims, rows, P):
    """Each listed row's global indices along the reduced dims, from its layer and offset."""
    n_coords = [len(d) for d in dims[:P]]
    cstride = [int(np.prod(CHUNKS[d + 1:])) for d in range(3)]
    out = []
    for layer, off in zip(rows.layer.tolist(), rows.offset.tolist()):
        coords = np.unravel_index(layer, n_coords)
        g = []
        for d in range(P):
            li = off // cstride[d] % CHUNKS[d]
            g.append(dims[d][coords[d]].chunk_ix * CHUNKS[d] + li)
        assert off == sum((x % CHUNKS[d]) * cstride[d] for d, x in enumerate(g))   # nothing of a kept dim in it
        out.append(tuple(g))
    return out


def test_row_list_sorted_stable_and_runs():
    labels = np.arange(15) % 3
    dims, rows = _rows((Ellipsis,), labels, 0, 1, 3)
    got = [g[0] for g in _global_rows(dims, rows, 1)]
    assert got == [0, 3, 6, 9, 12, 1, 4, 7, 10, 13, 2, 5, 8, 11, 14]       # by label, increasing inside a label
    assert rows.label.tolist() == [0] * 5 + [1] * 5 + [2] * 5 and rows.n_rows == 15
    assert rows.starts.tolist() == [0, 5, 10, 15]
    assert rows.layer.tolist() == [int(x >= 8) for x in got]
    assert rows.offset.tolist() == [(x % 8) * 12 * 20 for x in got]
    assert all(a.dtype == np.int32 for a in (rows.layer, rows.offset, rows.label))


def test_row_list_excluded_rows_are_absent_and_empty_groups_have_empty_runs():
    labels = np.array([4, -1, 1, 1, -7, 4, -1, -1, -1, -1, -1, -1, -1, -1, 1])    # layer 1 holds one listed row
    dims, rows = _rows((Ellipsis,), labels, 0, 1, 7)
    assert [g[0] for g in _global_rows(dims, rows, 1)] == [2, 3, 14, 0, 5]
    assert rows.label.tolist() == [1, 1, 1, 4, 4]
    assert rows.starts.tolist() == [0, 0, 3, 3, 3, 5, 5, 5]
    assert rows.layer.tolist() == [0, 0, 1, 0, 0]
    # every label negative: no row at all
    _, none = _rows((Ellipsis,), np.full(15, -1), 0, 1, 0)
    assert none.n_rows == 0 and none.starts.tolist() == [0]
    # a box that leaves a layer without a selected row: that layer contributes none
    dims, rows = _rows((slice(9, 13),), np.arange(15) % 2, 0, 1, 2)
    assert len(dims[0]) == 1 and set(rows.layer.tolist()) == {0}
    assert [g[0] for g in _global_rows(dims, rows, 1)] == [10, 12, 9, 11]
    assert rows.offset.tolist() == [2 * 240, 4 * 240, 1 * 240, 3 * 240]


@pytest.mark.parametrize("index", [(slice(1, None, 3),), ([13, 2, 3, 9, 0],)], ids=["stride", "list"])
def test_row_list_takes_the_labels_at_the_global_indices(index):
    labels = np.array([2, 0, 1, 1, 0, 2, 2, 0, 1, -1, 0, 2, 1, 0, 2])
    dims, rows = _rows(index, labels, 0, 1, 3)
    sel = np.arange(15)[index[0]]
    got = [g[0] for g in _global_rows(dims, rows, 1)]
    want = [int(i) for g in range(3) for i in sorted(sel[labels[sel] == g])]
    assert got == want and rows.label.tolist() == [int(labels[i]) for i in want]


def test_row_list_two_reduced_dims():
    """axis=(0, 1), labels along dim 1: every (row of dim 0, row of dim 1) pair
    once, C order over the global indices inside a label."""
    labels = np.arange(22) // 5        # 0 .. 4, the last group two rows
    labels[7] = -1
    index = (slice(3, 12), slice(2, 21), slice(None))
    dims, rows = _rows(index, labels, 1, 2, 5)
    got = _global_rows(dims, rows, 2)
    want = [(i, j) for g in range(5) for i in range(3, 12) for j in range(2, 21) if labels[j] == g]
    assert got == want
    assert rows.starts.tolist() == np.searchsorted([labels[j] for _, j in want], np.arange(6)).tolist()
    assert set(rows.layer.tolist()) == {0, 1, 2, 3}


# -- the walk path's lists and segments -----------------------------------------
def _emulate_walk(data, index, labels, along, axes, n_groups):
    """The walk path in NumPy: per chunk and local group the selected elements
    through the CSR lists, merged over the segments in ``order``."""
    ix = OrthogonalIndexer(index, data.shape, CHUNKS)
    final_shape = tuple(1 if d in axes else n for d, n in enumerate(ix.shape))
    chunk_list = list(ix)
    cl = grouped.chunk_lists((p for _, p in chunk_list), CHUNKS, labels, along, axes, final_shape, n_groups)
    recs = []
    for c, (coords, projs) in enumerate(chunk_list):
        local = [grouped._local(p) for p in projs]
        block = data[np.ix_(*[li + cc * ch for li, cc, ch in zip(local, coords, CHUNKS)])]   # the chunk's selection
        for j in range(cl.chunk_start[c], cl.chunk_start[c + 1]):
            pos = cl.pos[cl.ptr[j]:cl.ptr[j + 1]]
            assert np.all(np.diff(pos) > 0)
            sub = np.take(block, pos, axis=along)
            red = sub.sum(axis=tuple(axes), keepdims=True), np.prod([sub.shape[d] for d in axes])
            kept = red[0].reshape(-1)
            recs.append(np.stack([kept, np.full(kept.size, red[1])], axis=1))
        assert cl.out_off[c + 1] - cl.out_off[c] == sum(r.shape[0] for r in recs) - cl.out_off[c]
    recs = np.concatenate(recs) if recs else np.zeros((0, 2))
    rshape = tuple(n_groups if d == along else n for d, n in enumerate(final_shape))
    out = np.zeros((int(np.prod(rshape)), 2))
    for f in range(out.shape[0]):
        idx = cl.order[cl.seg[f]:cl.seg[f + 1]]
        assert np.all(np.diff(idx) > 0)            # in chunk order
        out[f] = recs[idx].sum(axis=0)
    return out.reshape(rshape + (2,)), cl


def _direct(data, index, labels, along, axes, n_groups, numpy_index=None):
    sel = data[np.ix_(*[np.arange(n)[i] for n, i in zip(data.shape, numpy_index or index)])]
    lab = labels[np.arange(data.shape[along])[(numpy_index or index)[along]]]
    parts = []
    for g in range(n_groups):
        sub = np.take(sel, np.nonzero(lab == g)[0], axis=along)
        s = sub.sum(axis=tuple(axes), keepdims=True)
        n = np.full(s.shape, np.prod([sub.shape[d] for d in axes]), dtype=np.float64)
        parts.append(np.stack([s, n], axis=-1))
    return np.concatenate(parts, axis=along)


WALK_CASES = [
    ("box-along0", (slice(1, -1), slice(1, -1), slice(1, -1)), 0, (0,)),
    ("box-along1-notprefix", (slice(None), slice(None), slice(None)), 1, (1,)),
    ("box-along2", (slice(None), slice(2, 20), slice(None)), 2, (2,)),
    ("box-all-dims", (slice(None), slice(None), slice(None)), 0, (0, 1, 2)),
    ("stride-along", (slice(1, None, 3), slice(None), slice(None)), 0, (0, 2)),
    ("list-along", ([13, 2, 3, 9, 0], slice(None), slice(3, 30)), 0, (0,)),
    ("list-kept", (slice(None), [0, 5, 6, 21], slice(None)), 0, (0, 1)),
]


@pytest.mark.parametrize("name,index,along,axes", WALK_CASES, ids=[c[0] for c in WALK_CASES])
def test_chunk_lists_reproduce_the_selection(name, index, along, axes):
    rng = np.random.default_rng(5)
    data = rng.integers(0, 1000, SHAPE).astype(np.float64)     # integer sums: exact in any order
    labels = rng.integers(-1, 4, SHAPE[along])
    labels[labels == 2] = 3                                    # group 2 is empty, group 4 beyond the labels
    got, cl = _emulate_walk(data, index, labels, along, axes, 5)
    want = _direct(data, index, labels, along, axes, 5)
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert not got.take(2, axis=along)[..., 1].any() and not got.take(4, axis=along)[..., 1].any()
    assert cl.chunk_start.dtype == np.int32 and cl.ptr.dtype == np.int32 and cl.pos.dtype == np.int32
    assert cl.seg.size == int(np.prod(want.shape[:-1])) + 1 and cl.order.size == cl.out_off[-1]
    assert (cl.group_label >= 0).all() and 2 not in cl.group_label


def test_chunk_lists_positions_are_among_the_selected_indices():
    """A listed selection in another order: position k is the k-th entry of the
    chunk's selection, not an index inside the chunk."""
    labels = np.arange(15) % 2
    index = ([14, 1, 6, 3, 8], slice(0, 1), slice(0, 1))
    ix = OrthogonalIndexer(index, SHAPE, CHUNKS)
    chunk_list = list(ix)
    cl = grouped.chunk_lists((p for _, p in chunk_list), CHUNKS, labels, 0, (0,), (1, 1, 1), 2)
    # chunk 0 selects [1, 6, 3] (labels 1, 0, 1), chunk 1 [14 - 8, 8 - 8] = global 14, 8 (labels 0, 0)
    assert cl.chunk_start.tolist() == [0, 2, 3]
    assert cl.group_label.tolist() == [0, 1, 0]
    assert [cl.pos[a:b].tolist() for a, b in zip(cl.ptr[:-1], cl.ptr[1:])] == [[1], [0, 2], [0, 1]]
    assert cl.out_off.tolist() == [0, 2, 3]
    assert cl.order.tolist() == [0, 2, 1] and cl.seg.tolist() == [0, 2, 3]


# -- finalize -------------------------------------------------------------------
def test_finalize_masks():
    parts = moments.records([[3, 1, 0]], [[2.0, 5.0, 0.0]], [[6.0, 0.0, 0.0]])
    mean = grouped.finalize(parts, "mean")
    assert mean.dtype == np.float64 and mean.shape == (1, 3)
    assert np.ma.getmaskarray(mean).tolist() == [[False, False, True]] and mean.data.tolist() == [[2.0, 5.0, 0.0]]
    var0, var1 = grouped.finalize(parts, "var", 0), grouped.finalize(parts, "var", 1)
    assert np.ma.getmaskarray(var0).tolist() == [[False, False, True]] and var0.data.tolist() == [[2.0, 0.0, 0.0]]
    assert np.ma.getmaskarray(var1).tolist() == [[False, True, True]] and var1.data[0, 0] == 3.0
    std = grouped.finalize(parts, "std", 1)
    assert std.data[0, 0] == np.sqrt(3.0)
    assert grouped.finalize(parts, "var", 1).tobytes() == moments.finalize(parts, 1).tobytes()
    cnt = grouped.finalize(parts, "count")
    assert type(cnt) is np.ndarray and cnt.dtype == np.int64 and cnt.tolist() == [[3, 1, 0]]
    nan = grouped.finalize(moments.records([2], [np.nan], [np.nan]), "mean")
    assert not np.ma.getmaskarray(nan).any() and np.isnan(nan.data).all()
    with pytest.raises(ValueError):
        grouped.finalize(parts, "median")


# -- Active's argument checks -------------------------------------------------------
def test_api_returns_self_and_holds_the_settings():
    a = Active(_var())
    assert a.grouped("var", 0, [0, 1], axis=(0,), ddof=1) is a
    assert a._method == "grouped" and a._ddof == 1 and a._axis == (0,)
    assert a._grouped["stat"] == "var" and a._grouped["along"] == 0 and a._grouped["n_groups"] == 2
    assert a.grouped("mean", -1, [0, 0, 3, -1], n_groups=6) is a
    assert a._grouped["along"] == 2 and a._grouped["n_groups"] == 6 and a._ddof == 0
    assert a.grouped_path is None
    a.method = "mean"
    assert a._grouped is None


@pytest.mark.parametrize("kw", [
    dict(stat="median", along=0, labels=[0, 1]),
    dict(stat="mean", along=3, labels=[0, 1]),
    dict(stat="mean", along=-4, labels=[0, 1]),
    dict(stat="mean", along=True, labels=[0, 1]),
    dict(stat="mean", along=0.0, labels=[0, 1]),
    dict(stat="mean", along=0, labels=[0.0, 1.0]),
    dict(stat="mean", along=0, labels=[True, False]),
    dict(stat="mean", along=0, labels=[0, 1, 2]),
    dict(stat="mean", along=1, labels=[0, 1]),              # dim 1 has 3 entries
    dict(stat="mean", along=0, labels=[0, 2], n_groups=2),
    dict(stat="var", along=0, labels=[0, 1], ddof=-1),
    dict(stat="var", along=0, labels=[0, 1], ddof=1.5),
])
def test_bad_arguments(kw):
    with pytest.raises(ValueError):
        Active(_var()).grouped(**kw)


def test_query_time_errors_before_any_device_call(monkeypatch):
    from pyactivestorage_amd import active as mod

    def no_device(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(mod, "get_context", no_device)
    a = Active(_var(), group=object())
    with pytest.raises(NotImplementedError, match="grouped with group="):
        a.grouped("mean", 0, [0, 1], axis=(0,))[...]
    assert a._grouped is None and a._method is None        # the settings hold for one query
    a = Active(_var())
    with pytest.raises(ValueError, match="grouped: along=0 is not among the reduced axes"):
        a.grouped("mean", 0, [0, 1], axis=(1,))[...]
    with pytest.raises(ValueError, match="weights apply to mean and sum only"):
        a.weights = {0: [1.0, 2.0]}
        a.grouped("mean", 0, [0, 1], axis=(0,))[...]
    assert a._weights is None and a._grouped is None
    with pytest.raises(IndexError, match="drops the axis"):
        a.grouped("mean", 0, [0, 1], axis=(0,))[:, 1]
    # no group, or no selected element: the result without a launch
    got = a.grouped("mean", 0, [-1, -1], axis=(0,))[...]
    assert isinstance(got, np.ma.MaskedArray) and got.shape == (0, 3, 4) and got.dtype == np.float64
    got = a.grouped("count", 0, [0, 1], axis=(0,), n_groups=3)[:, 1:1]
    assert type(got) is np.ndarray and got.shape == (3, 0, 4) and got.dtype == np.int64
    assert a.grouped_path is None


def test_record_cap(monkeypatch):
    from pyactivestorage_amd import active as mod
    monkeypatch.setattr(mod, "get_context", lambda *a, **k: (_ for _ in ()).throw(AssertionError("device call")))
    monkeypatch.setattr(mod.histogram, "TABLE_CAP_BYTES", 12 * 2 * _lib.MOMENTS_NBYTES - 1)
    a = Active(_var())
    with pytest.raises(ValueError, match="above the cap"):
        a.grouped("mean", 0, [0, 1], axis=(0,))[...]


def test_itertools_product_matches_the_box_plan_order():
    """The walk path of a box query lists its chunks as the product of the
    per-dim projections: the order of the box plan's chunk coordinates."""
    ix = OrthogonalIndexer((slice(None), slice(None), slice(None)), SHAPE, CHUNKS)
    dims = [list(d) for d in ix.dim_indexers]
    got = [tuple(p.chunk_ix for p in projs) for projs in itertools.product(*dims)]
    assert got == [c for c, _ in ix]
    assert engine.moments_dtype.itemsize == _lib.MOMENTS_NBYTES
