"""Shapes and data of the branch-coverage cases shared by the eight statistics
modules.  ``test_gpu_moments``, ``test_gpu_weighted``, ``test_gpu_histogram``,
``test_gpu_quantile`` and ``test_gpu_comoments`` run them themselves.  The
cases of ``test_gpu_trend``, ``test_gpu_grouped`` and
``test_gpu_grouped_extremes`` are run by ``test_stats_gaps_trend``,
``test_stats_gaps_grouped`` and ``test_stats_gaps_grouped_extremes``, each
with the ``make_var`` / ``oracle`` / ``check`` / ``query`` it imports from
the module it is named for.  Every case goes through its statistic's own
oracle and bound; nothing here touches the device except
:func:`misaligned_plan`.

The cases, by the branch they reach (``tests/test_stats_gap_shapes.py`` checks
the shapes against the constants in ``csrc``):

G1  reduced positions on both sides of the LDS offset map (``kMomRoff`` /
    ``kComRoff``): the radix-counter walk of ``k_moments_axes`` and
    ``k_comoments_axes`` with a wave and with a lane per output.
G2  more kept outputs in one chunk than ``LAUNCH_CAP x kBlock``: the second
    trip of the lane-per-output loop of every ``*_axes`` kernel.
G3  byte-shuffled chunks whose element count is no multiple of 16 (the
    per-element fallback of the shuffled runs), and runs of a shuffled chunk
    that start and end inside a 16-element group or are shorter than one.
G4  ranks 1, 2, 4 and 8 (``PYAS_MAX_DIMS``).
G5  the dtypes the sweeps leave out, byte-swapped 2- and 8-byte types, and
    uint64 values at and above 2^63.
G6  chunk bases that are not 16-byte aligned, through the C entry points.

The three ``test_stats_gaps_*`` modules run G2 to G5 through :func:`runs`, which adds the
queries that take their dense column kernels (``k_trend_cols``,
``k_group_cols``, ``k_group_cols_partial``), and these cases of their own:

T1  G1 for ``k_trend_axes``: reduced positions on both sides of ``kTrendRoff``,
    with zero and non-zero starts, a wave and a lane per output.
T2  more reduced rows in one chunk layer than ``k_trend_cols`` stages per pass
    (``kTrendRows``), and exactly as many; one and two reduced dims.
C1  more items in a column of chunks than ``kBlock``: several workgroups per
    column in the dense kernels, the last with idle lanes, and columns whose
    later workgroups have nothing to do.
M   the mask modes the sweeps do not dispatch: both equality rules with both
    thresholds, a lone ``missing_value``, a lone ``valid_max``.
G6D chunk bases that are not ``kAlign``-aligned under the dense kernels'
    4-element loads, through the C entry points.
"""
import functools
import itertools

import numpy as np

from oracle import storage_ref as ref

# Workgroups per chunk of a partial-axes launch.  The cap has no name in the
# source: it is the literal 64 in pyas_moments_axes, pyas_comoments_axes and
# pyas_wsum_axes, and in hist_axes_shape (which pyas_hist_axes and
# pyas_select_axes share), all in csrc/pyas_capi.hip.
LAUNCH_CAP = 64

QS = [0, 0.3, 0.5, 1]
HIST_BINS, HIST_RANGE = 4, (270.0, 300.0)     # f4 / f8 N(288, 10): edges 270, 277.5, 285, 292.5, 300

ALL = (Ellipsis,)


def axis_id(axis):
    return "all" if axis is None else "".join(map(str, axis))


# -- the cases -----------------------------------------------------------------
# name -> (shape, chunks, axes, {index name: index}, shuffled)
G1 = {
    # first chunk 17 x 241 = 4,097 reduced positions (the walk), edge chunk 13 x 241 = 3,133 (the map)
    "row": ((30, 2, 241), (17, 2, 241), [(0, 2)],
            {"whole": ALL, "from": (slice(1, None), slice(None), slice(3, None))}, False),
    # 4,096: the last mapped size
    "map": ((64, 2, 64), (64, 2, 64), [(0, 2)],
            {"whole": ALL, "from": (slice(1, None), slice(None), slice(3, None))}, False),
    # the same with the innermost dim kept: a lane per output
    "lane": ((30, 241, 2), (17, 241, 2), [(0, 1)],
             {"whole": ALL, "from": (slice(1, None), slice(3, None), slice(None))}, False),
    # "from" leaves 16 x 238 = 3,808 positions of the chunks above: mapped.  Here it leaves
    # 17 x 247 = 4,199, so the walk also runs with non-zero starts (the edge chunk: 13 x 247, mapped)
    "row-from": ((31, 2, 250), (18, 2, 250), [(0, 2)],
                 {"from": (slice(1, None), slice(None), slice(3, None))}, False),
    "lane-from": ((31, 250, 2), (18, 250, 2), [(0, 1)],
                  {"from": (slice(1, None), slice(3, None), slice(None))}, False),
}
G2 = {
    # 130 x 130 = 16,900 kept outputs of 3 (6) elements each; LAUNCH_CAP x kBlock = 16,384
    "one": ((3, 130, 130), (3, 130, 130), [(0,)], {"whole": ALL}, False),
    "two": ((6, 130, 130), (3, 130, 130), [(0,)], {"whole": ALL}, False),
}
G2_SECOND_TRIP = 16384      # outputs from here on belong to the loop's second trip
G3 = {
    # 105 elements per chunk; edge chunks in every dim
    "odd": ((5, 9, 13), (3, 5, 7), [None, (0,), (2,)], {"whole": ALL, "from1": (slice(1, None), Ellipsis)}, True),
    # the weighted full reduction walks chunks whose rows are shorter than a vector of 16: rows of 17
    # (255 elements per chunk) put its shuffled run on the per-element fallback
    "odd17": ((5, 9, 33), (3, 5, 17), [None, (0,), (2,)], {"whole": ALL, "from1": (slice(1, None), Ellipsis)}, True),
    # 320 elements (a multiple of 16) in one chunk; contiguous runs of chunk elements
    "runs": ((4, 4, 20), (4, 4, 20), [None],
             {"80-320": (slice(1, 4), slice(None), slice(None)),       # whole groups
              "20-60": (slice(0, 1), slice(1, 3), slice(None)),        # starts and ends inside a group
              "3-12": (slice(0, 1), slice(0, 1), slice(3, 12))},       # shorter than a group
             True),
}
G3_DTYPES = ["<f4", "<f8", "<i2"]
G3_RUNS = {"80-320": (80, 320), "20-60": (20, 60), "3-12": (3, 12)}
_R8 = (3, 2, 3, 2, 3, 2, 3, 5)
_STRIDED = (slice(None, None, 2), Ellipsis)
G4 = {
    "1d": ((1000,), (300,), [None, (0,)], {"whole": ALL, "strided": _STRIDED}, False),
    "2d": ((37, 45), (20, 31), [None, (0,), (1,)], {"whole": ALL, "strided": _STRIDED}, False),
    "4d": ((5, 6, 7, 33), (3, 4, 4, 20), [None, (0,), (3,)], {"whole": ALL, "strided": _STRIDED}, False),
    # 3,240 elements in 32 chunks, edge chunks in five dims
    "8d": (_R8, (2, 2, 2, 2, 2, 2, 2, 3), [None, (7,), (0,), (1, 3, 5, 7), (0, 2, 4, 6)],
           {"whole": ALL, "strided": _STRIDED}, False),
}
G5 = {"dtypes": ((9, 14, 33), (4, 8, 16), [None, (1,)], {"whole": ALL}, False)}
G5_DTYPES = ["<u8", "<i4", "<u4", "<u2", "|i1", ">i2", ">f8", ">i8"]
G5_LAYOUTS = [(dt, sh) for dt in G5_DTYPES for sh in ((False, True) if dt[0] == ">" else (False,))]
G5_HIST_RANGE = {     # four bins inside each type's spread
    "<u8": (2.0 ** 62, 3 * 2.0 ** 62), "<i4": (-1.0e9, 1.0e9), "<u4": (1.0e9, 3.0e9), "<u2": (16000, 48000),
    "|i1": (-50, 50), ">i2": (-1500, 1500), ">f8": HIST_RANGE, ">i8": (-2.0 ** 55, 2.0 ** 55),
}
U8_FILL, U8_MAX, U8_MIN = 2 ** 64 - 1, 2 ** 64 - 2 ** 20, 2 ** 10
# Outside the two bounds, and the bounds themselves (kept).  2^64 - 2^20 + 1 converts to the
# float64 2^64 - 2^20: a comparison made after conversion would keep it.
U8_PLANTS = [0, 5, U8_MIN - 1, U8_MAX + 1, U8_MAX + 2 ** 19, 2 ** 64 - 2, U8_MIN, U8_MAX]
G6_SHAPE = (33, 65, 31)
G6_OFFSETS = {"<f4": (4, 8, 12), "|u1": (1, 15)}
G6_INDEXES = {"whole": None, "from1": (slice(1, None), slice(None), slice(None))}


# -- the cases of the trend and grouped modules ----------------------------------
HUGE = 1e30                  # planted in the float chunks' padding: one element of it read shows in any result
G2_WALK = {"one": (list(range(3)),), "two": (list(range(6)),)}     # every row, listed: not a box, so the walk
G3_WALK = (slice(None), slice(None, None, 2), slice(None))
G4_PREFIXES = {"1d": [], "2d": [(0,)], "4d": [(0,)], "8d": [(0,), (0, 1, 2, 3), (0, 1, 2, 3, 4, 5, 6)]}
_LISTED = [0, 1]             # both positions of a dim of extent 2, listed
T1 = {
    # first chunk 3 x 683 = 2,049 reduced positions (the walk), edge chunk 2 x 683 = 1,366 (the map)
    "row": ((5, 2, 683), (3, 2, 683), [(0, 2)], {"whole": ALL}, False),
    # the same with the innermost dim kept: a lane per output.  (0, 1) is a leading prefix, so the
    # whole variable takes the dense kernel (3 x 683 rows a layer: two staging passes over two
    # reduced dims); with the innermost dim listed the query is no box and takes the walk
    "lane": ((5, 683, 2), (3, 683, 2), [(0, 1)],
             {"whole": ALL, "listed": (slice(None), slice(None), _LISTED)}, False),
    # 2,048: the last mapped size
    "map": ((32, 2, 64), (32, 2, 64), [(0, 2)], {"whole": ALL}, False),
    # 3 x 683 = 2,049 positions again, with non-zero starts (the edge chunk: 2 x 683, mapped)
    "row-from": ((6, 2, 690), (4, 2, 690), [(0, 2)], {"from": (slice(1, None), slice(None), slice(7, None))}, False),
    "lane-from": ((6, 690, 2), (4, 690, 2), [(0, 1)], {"from": (slice(1, None), slice(7, None), _LISTED)}, False),
}
T2 = {
    # layer 0 has 1,061 rows (a pass of 1,024 and one of 37), layer 1 exactly 1,024; from row 37
    # on both layers have exactly 1,024 and layer 0 a non-zero start
    "rows": ((2085, 2, 8), (1061, 2, 8), [(0,)], {"whole": ALL, "from37": (slice(37, None), Ellipsis)}, False),
    # 35 x 30 = 1,050 rows over two reduced dims: row 1,024 is (34, 4), inside a row of dim 1
    "p2": ((40, 30, 8), (35, 30, 8), [(0, 1)], {"whole": ALL}, False),
}
C1 = {
    # 9 x 30 = 270 items in the two full columns (bpc 2, 14 live lanes in the second workgroup),
    # 27, 60 and 6 in the edge columns; the box cuts the first column to 8 x 30 = 240
    "wg2": ((7, 20, 132), (4, 9, 120), [(0,)],
            {"whole": ALL, "box": (slice(1, 6), slice(1, 19), slice(2, 131))}, False),
    # 18 x 30 = 540 items (bpc 3), two reduced dims and a kept dim between them and the innermost
    "wg3-4d": ((5, 5, 20, 132), (2, 3, 18, 120), [(0, 1)], {"whole": ALL}, False),
}
T_DTYPES = {"T1": ["<f4"], "T2": ["<f4", "|u1"], "C1": ["<f4", "<i2"]}

GROUPS = {"G1": G1, "G2": G2, "G3": G3, "G4": G4, "G5": G5, "T1": T1, "T2": T2, "C1": C1}


def case(group, name):
    return GROUPS[group][name]


def combos(group, name):
    """Every ``(index name, index, axis, least valid elements per output)`` of a case."""
    shape, chunks, axes, indexes, _ = case(group, name)
    out = []
    for iname, index in indexes.items():
        for axis in axes:
            need = 2 if group in ("G2", "G4", "T1", "T2", "C1") else 0
            if (group, name, iname, axis) == ("G4", "8d", "strided", (0,)):
                need = 1       # two elements per output: a masked one leaves a single valid element
            out.append((iname, per_dim(index, len(shape)), axis, need))
    return out


def index_of(group, name, iname):
    """A case's index, a slice per dim."""
    shape, _, _, indexes, _ = case(group, name)
    return per_dim(indexes[iname], len(shape))


# -- data ------------------------------------------------------------------------
def _field(dt, shape, rng):
    """x by dtype: floats N(288, 10); integers over (nearly) their whole
    range, signed ones on both sides of zero; ``(x, fill)``."""
    dt = np.dtype(dt)
    nat = dt.newbyteorder("=")
    if dt.kind == "f":
        return rng.normal(288.0, 10.0, shape).astype(dt), -999.0
    if nat == np.dtype(np.uint64):
        return rng.integers(0, 2 ** 64 - 1, shape, dtype=np.uint64, endpoint=False).astype(dt), U8_FILL
    if nat == np.dtype(np.int64):     # odd values up to 2^56 in magnitude, about zero (see the moments sweep)
        return (rng.integers(-2 ** 55, 2 ** 55, shape) * 2 + 1).astype(dt), -2 ** 63
    if nat == np.dtype(np.int16):
        return rng.integers(-3000, 3000, shape).astype(dt), -32768
    info = np.iinfo(nat)
    if dt.kind == "i":                # the fill is the type's minimum, which the data never take
        return rng.integers(info.min + 1, info.max, shape, endpoint=True).astype(dt), info.min
    return rng.integers(0, info.max, shape).astype(dt), info.max


def _partner(x, rng):
    """y = 0.3 x + noise (r about 0.5) in x's dtype."""
    dt = x.dtype
    nat = dt.newbyteorder("=")
    xf = x.astype(np.float64)
    if dt.kind == "f":
        return (0.3 * xf + rng.normal(0.0, 5.2, x.shape)).astype(dt)
    sd = float(xf.std())
    if nat.itemsize == 8:
        lo, hi = (0.0, 2.0 ** 64 - 2.0 ** 13) if dt.kind == "u" else (-2.0 ** 62, 2.0 ** 62)
    else:
        info = np.iinfo(nat)
        lo, hi = float(info.min + 1), float(info.max - 1)
    centre = 0.35 * hi if dt.kind == "u" else 0.0
    y = np.clip(np.rint(0.3 * xf + centre + rng.normal(0.0, 0.52 * sd, x.shape)), lo, hi).astype(nat)
    if nat == np.dtype(np.uint64):    # float64 values are multiples of 2^11 up here: odd low bits again
        y = y + rng.integers(0, 2 ** 11, x.shape, dtype=np.uint64)
    return y.astype(dt)


def valid_counts(mask, index, axis):
    return (~mask)[index].sum(axis=axis, keepdims=True)


def _mask_positions(shape, rng, n_x, n_y, guard):
    """``n_x`` positions for x's fill values and ``n_y`` others for y's, taken
    in a random order; a position is passed over when masking it would leave
    an output of ``guard`` (``(index, axis, need)``) with fewer than ``need``
    elements valid on both sides."""
    size = int(np.prod(shape))
    mask = np.zeros(shape, bool)
    flat = mask.reshape(-1)
    took = []
    for pos in rng.permutation(size):
        if len(took) == n_x + n_y:
            break
        flat[pos] = True
        if all(valid_counts(mask, index, axis).min() >= need for index, axis, need in guard if need):
            took.append(pos)
        else:
            flat[pos] = False
    assert len(took) == n_x + n_y
    return np.array(took[:n_x], np.int64), np.array(took[n_x:], np.int64)


def _one(v, dt):
    return np.array([v], dtype=np.dtype(dt).newbyteorder("="))


@functools.lru_cache(maxsize=None)
def pair(group, name, dt="<f4", masked=False):
    """``(x, y, attrs_x, attrs_y)`` of a case, read-only.  Masked: a scalar
    ``_FillValue`` at 2 % of x's elements and at another 3 % of y's.  The
    single-variable statistics use ``x`` and ``attrs_x``.  ``<u8``: x also has
    ``valid_min`` / ``valid_max`` and values outside both."""
    shape = case(group, name)[0]
    seed = sum(map(ord, group + name + np.dtype(dt).str)) * 2 + masked
    rng = np.random.default_rng(seed)
    x, fill = _field(dt, shape, rng)
    y = _partner(x, rng)
    ax, ay = {}, {}
    if masked:
        guard = [(index, axis, need) for _, index, axis, need in combos(group, name)]
        px, py = _mask_positions(shape, rng, x.size // 50, 3 * x.size // 100, guard)
        x.reshape(-1)[px] = fill
        y.reshape(-1)[py] = fill
        ax, ay = {"_FillValue": _one(fill, dt)}, {"_FillValue": _one(fill, dt)}
        if np.dtype(dt).newbyteorder("=") == np.dtype(np.uint64):
            ax.update(valid_min=_one(U8_MIN, dt), valid_max=_one(U8_MAX, dt))
            free = np.setdiff1d(np.arange(x.size), np.concatenate([px, py]))
            plants = np.array(U8_PLANTS * 3, dtype=np.uint64)
            x.reshape(-1)[rng.choice(free, plants.size, replace=False)] = plants
    x.setflags(write=False)
    y.setflags(write=False)
    return x, y, ax, ay


def single(group, name, dt="<f4", masked=False):
    x, _, ax, _ = pair(group, name, dt, masked)
    return x, ax


def fill_of(attrs, dt):
    """The value edge chunks are padded with: the fill value where there is one."""
    if attrs:
        return attrs["_FillValue"][0]
    return np.dtype(dt).newbyteorder("=").type(0)


def pad_of(dt):
    """The value the trend and grouped cases pad edge chunks with: 1e30 for
    floats, the type's maximum for integers.  Never 0 and never inside the
    data's spread, so a lane that reads padding, or another lane's item,
    shows in a sum, a mean or a slope; it is above every valid datum of the
    T1, T2, C1, G2, G3 and G4 fields, so there it shows in a max as well.
    G5's integer fields span their types, so no value lies beyond them: there
    the padding can only equal the largest datum.  An unsigned type's maximum
    is also its fill value, so in a masked unsigned case a padding element is
    masked, and only the plain variant shows a read of it."""
    nat = np.dtype(dt).newbyteorder("=")
    return HUGE if nat.kind == "f" else np.iinfo(nat).max


@functools.lru_cache(maxsize=4)
def variable(make_var, group, name, dt="<f4", masked=False, shuffle=None):
    """``(x, attrs, variable)`` of a case for the trend and grouped modules:
    ``make_var`` is the module's own, the edge chunks are padded with
    :func:`pad_of`, and ``shuffle`` overrides the case's (1-byte types are
    never shuffled)."""
    x, attrs = single(group, name, dt, masked)
    chunks, shuffled = case(group, name)[1], case(group, name)[4]
    shuffle = (shuffled if shuffle is None else shuffle) and x.dtype.itemsize > 1
    return x, attrs, make_var(x, chunks, attrs, shuffle=shuffle, pad=pad_of(dt))


def _unit_box(index):
    return all(isinstance(ix, slice) and ix.step in (None, 1) for ix in index)


def is_prefix(axis, ndim):
    return axis is not None and len(axis) < ndim and tuple(sorted(axis)) == tuple(range(len(axis)))


def runs(group, name):
    """The queries the trend and grouped modules run of a case: ``(index name,
    index, axis, along, path)``, ``along`` the dim of the coordinate or of the
    labels and ``path`` the kernel the query takes, ``"cols"`` for a unit-step
    box reduced over a leading prefix of the dims, else ``"walk"``."""
    shape, _, axes, indexes, _ = case(group, name)
    nd = len(shape)
    indexes = dict(indexes)
    alongs = lambda axis: [0]
    if group == "G2":
        axes, indexes["listed"] = [(0,)], G2_WALK[name]
    elif group == "G3":
        axes, indexes["stride"] = [(0,)], G3_WALK
    elif group == "G4":       # the first and the last reduced dim
        axes = axes + [a for a in G4_PREFIXES[name] if a not in axes]
        alongs = lambda axis: sorted({(axis or range(nd))[0], (axis or range(nd))[-1]})
    elif group == "G5":
        axes, alongs = [(1,), (0,)], lambda axis: [axis[0]]
    elif (group, name) in (("T1", "row"), ("T2", "p2"), ("C1", "wg3-4d")):
        alongs = lambda axis: [0, axis[-1]]
    out = []
    for iname, index in indexes.items():
        index = per_dim(index, nd)
        for axis in axes:
            for along in alongs(axis):
                out.append((iname, index, axis, along, "cols" if _unit_box(index) and is_prefix(axis, nd) else "walk"))
    return out


def run_id(run):
    return f"{run[0]}-{axis_id(run[2])}-along{run[3]}"


def trend_points(mask, index, axis, along):
    """The least number, over the outputs, of distinct positions along
    ``along`` that hold a valid element: a slope needs two."""
    ok = ~np.asarray(mask)[index]
    axis = tuple(range(ok.ndim)) if axis is None else axis
    others = tuple(d for d in axis if d != along)
    has = ok.any(axis=others, keepdims=True) if others else ok
    return int(has.sum(axis=along, keepdims=True).min())


# -- M: mask modes -----------------------------------------------------------------
M_SHAPE, M_CHUNKS = (9, 14, 33), (4, 8, 16)
M_MODES = ("both", "missing", "max")
M_DTYPES = ["<f4", "<i2"]
M_INDEXES = {"whole": ALL, "stride": G3_WALK}
#        fill, missing_value, valid_min, valid_max, padding under a valid_max (valid, and no datum's neighbour:
#        both thresholds' own values are data, so nothing valid lies beyond them; with a lone missing_value
#        the padding is pad_of's, beyond every datum)
M_VALUES = {"<f4": (270.25, 300.5, 262.0, 314.0, 311.0), "<i2": (-1000, 1000, -2500, 2500, 2345)}


@functools.lru_cache(maxsize=None)
def mask_case(dt, mode):
    """``(x, attrs, pad, plants)``: ``both``: ``_FillValue`` and a scalar
    ``missing_value`` inside ``valid_min .. valid_max``, each at 2 % of the
    elements, the two thresholds' own values (kept: the bounds are inclusive)
    and their outer neighbours (masked) planted; ``missing``: ``missing_value``
    alone; ``max``: ``valid_max`` alone.  ``plants``: value -> masked or not."""
    d = np.dtype(dt)
    rng = np.random.default_rng(900 + 10 * M_DTYPES.index(dt) + M_MODES.index(mode))
    fill, miss, lo, hi, pad = M_VALUES[dt]
    if d.kind == "f":
        x = rng.normal(288.0, 10.0, M_SHAPE).astype(d)
        below, above = np.nextafter(d.type(lo), d.type(-np.inf)), np.nextafter(d.type(hi), d.type(np.inf))
    else:
        x = rng.integers(-3000, 3000, M_SHAPE).astype(d)
        below, above = lo - 1, hi + 1
    one = lambda v: np.array([v], dtype=d)
    pos = rng.permutation(x.size)
    n = x.size // 50
    f = x.reshape(-1)
    if mode == "both":
        attrs = {"_FillValue": one(fill), "missing_value": one(miss), "valid_min": one(lo), "valid_max": one(hi)}
        plants = {fill: True, miss: True, lo: False, hi: False, below: True, above: True}
        f[pos[:n]], f[pos[n:2 * n]] = fill, miss
        for k, v in enumerate((lo, hi, below, above)):
            f[pos[2 * n + 5 * k:2 * n + 5 * k + 5]] = v
    elif mode == "missing":
        attrs, plants = {"missing_value": one(miss)}, {miss: True}
        f[pos[:n]] = miss
    else:
        attrs, plants = {"valid_max": one(hi)}, {hi: False, above: True}
        f[pos[:5]], f[pos[5:10]] = hi, above
    x.setflags(write=False)
    return x, attrs, d.type(pad_of(dt) if mode == "missing" else pad), plants


# -- G6D: misaligned chunk bases under the dense kernels ------------------------------
G6D_SHAPE = (9, 5, 24)       # rows of 24 elements: whole-chunk items take the 4-element loads when the base allows
#            dtype, shuffled, byte offset, whether the 4-element loads still apply (kAlign divides the offset)
G6D_CASES = [("<f4", False, 4, False), ("<f4", False, 8, False), ("<f4", False, 12, False),
             ("<f4", True, 1, False), ("<f4", True, 2, False), ("<f4", True, 4, True),
             ("|u1", False, 1, False), ("|u1", False, 3, False), ("<i2", False, 2, False), ("<i2", False, 4, False)]
G6D_IDS = [f"{dt.replace('|', '=')}-{'shuffled' if sh else 'stored'}-{off}" for dt, sh, off, _ in G6D_CASES]
G6D_LABELS = np.array([1, 0, -1, 2, 2, 0, 1, 2, 0])     # three groups out of order and an excluded row


def k_align(dt, shuffled, v=4):
    """kAlign of the dense kernels (pyas_trend.hip, pyas_grouped.hip)."""
    es = np.dtype(dt).itemsize
    return 4 if shuffled and es > 1 else min(es * v, 16)


@functools.lru_cache(maxsize=None)
def g6d_chunk(dt):
    rng = np.random.default_rng(11)
    d = np.dtype(dt)
    i0 = np.arange(G6D_SHAPE[0])[:, None, None]
    if d.kind == "f":
        data = (rng.normal(288.0, 10.0, G6D_SHAPE) + 0.6 * i0).astype(d)
    elif d.itemsize == 1:
        data = (rng.integers(0, 200, G6D_SHAPE) + 3 * i0).astype(d)
    else:
        data = (rng.integers(-3000, 3000, G6D_SHAPE) + 40 * i0).astype(d)
    data.setflags(write=False)
    return data


def planted(data, attrs, values, seed=5):
    """A copy of ``data`` with ``values`` written over elements that are not fill values."""
    out = data.copy()
    flat = out.reshape(-1)
    free = np.arange(flat.size) if not attrs else np.nonzero(flat != attrs["_FillValue"][0])[0]
    rng = np.random.default_rng(seed)
    flat[rng.choice(free, len(values), replace=False)] = np.asarray(values).astype(data.dtype)
    out.setflags(write=False)
    return out


def weights(shape, dims=None, seed=8):
    rng = np.random.default_rng(seed)
    w = {d: rng.uniform(0.1, 3.0, n) for d, n in enumerate(shape)}
    return w if dims is None else {d: w[d] for d in dims}


@functools.lru_cache(maxsize=None)
def g6_chunk(dt, spread=False):
    """One (33, 65, 31) chunk: f4 N(288, 10), or N(0, 40) for the digit counts
    of the select (keys spread over many first digits); u1 over 0..255."""
    rng = np.random.default_rng(7)
    if np.dtype(dt).kind == "f":
        data = (rng.normal(0.0, 40.0, G6_SHAPE) if spread else rng.normal(288.0, 10.0, G6_SHAPE)).astype(dt)
    else:
        data = rng.integers(0, 256, G6_SHAPE).astype(dt)
    data.setflags(write=False)
    return data


G6_CASES = [(dt, off) for dt, offs in G6_OFFSETS.items() for off in offs]


def misaligned_plan(gpu, data, off, index=None, shuffle=False):
    """``data`` as one chunk ``off`` bytes into a device buffer of exactly
    ``off + data.nbytes`` bytes, and the ReductionPlan of ``index`` (None: the
    whole chunk) over it: ``(stream, buffer, plan)``.  ``shuffle``: the chunk
    is stored byte-shuffled; its byte planes may start at any byte, so ``off``
    need be no multiple of the element size then (the plan's data pointer
    carries the offset: the chunk's own offset must be a multiple)."""
    from pyactivestorage_amd import selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    st = gpu.thread_stream()
    raw = np.frombuffer(data.tobytes(), np.uint8)
    if shuffle:
        raw = raw.reshape(-1, data.dtype.itemsize).T.reshape(-1)
    host = np.zeros(off + data.nbytes, np.uint8)
    host[off:] = raw
    buf = DeviceBuffer(gpu, host.nbytes)
    assert buf.ptr % 16 == 0 and (buf.ptr + off) % 16 == off % 16 != 0
    gpu.h2d(buf.ptr, host, st)
    sels = None if index is None else [selection.normalize(index, data.shape)]
    ptr, offsets = (buf.ptr + off, [0]) if off % data.dtype.itemsize else (buf.ptr, [off])
    assert shuffle or ptr == buf.ptr
    plan = ReductionPlan(gpu, data.dtype, data.shape, ptr, np.array(offsets, np.int64), selections=sels,
                         shuffle=data.dtype.itemsize if shuffle else 0, missing=(None,) * 4, stream=st)
    return st, buf, plan


# -- what the shapes reach (host arithmetic, for tests/test_stats_gap_shapes.py) -----
def _dim_counts(n, c, ix):
    """Selected positions of a dim of extent ``n`` per chunk of ``c``."""
    sel = np.arange(n)[ix]
    return [int(((sel >= a) & (sel < a + c)).sum()) for a in range(0, n, c)]


def per_dim(index, ndim):
    index = index if isinstance(index, tuple) else (index,)
    if Ellipsis in index:
        k = index.index(Ellipsis)
        index = index[:k] + (slice(None),) * (ndim - len(index) + 1) + index[k + 1:]
    return index + (slice(None),) * (ndim - len(index))


def chunk_counts(shape, chunks, index, axis):
    """``(n_red, n_keep)`` of every touched chunk: the selected positions over
    the reduced and over the kept dims, as the ``*_axes`` kernels count them."""
    nd = len(shape)
    axis = tuple(range(nd)) if axis is None else axis
    per = [_dim_counts(n, c, ix) for n, c, ix in zip(shape, chunks, per_dim(index, nd))]
    out = []
    for cc in np.ndindex(*[len(p) for p in per]):
        cnt = [per[d][cc[d]] for d in range(nd)]
        if min(cnt) > 0:
            out.append((int(np.prod([cnt[d] for d in axis])), int(np.prod([cnt[d] for d in range(nd) if d not in axis]))))
    return out


def _dim_spans(n, c, ix):
    """``(first selected index inside the chunk, selected positions)`` of every
    touched chunk of a dim of extent ``n`` in chunks of ``c``."""
    sel = np.arange(n)[ix]
    out = []
    for a in range(0, n, c):
        loc = sel[(sel >= a) & (sel < a + c)] - a
        if loc.size:
            out.append((int(loc[0]), int(loc.size)))
    return out


def dense_columns(shape, chunks, index, axis, v, block):
    """``(n_items, bpc)`` of every column of chunks of a dense query (a
    unit-step box reduced over the leading dims ``axis``): the items ``KO x G``
    as k_trend_cols and k_group_cols count them from the column's selection
    (``v`` outputs per item, aligned to ``v`` elements of the chunk row), and
    the workgroups per column as pyas_trend_cols and group_cols_run count them
    from the chunk shape (``block`` items per workgroup)."""
    nd, P = len(shape), len(axis)
    index = per_dim(index, nd)
    assert is_prefix(axis, nd) and _unit_box(index)
    spans = [_dim_spans(shape[d], chunks[d], index[d]) for d in range(P, nd)]
    items = -(-chunks[-1] // v) * int(np.prod(chunks[P:nd - 1], dtype=np.int64))
    bpc = -(-items // block)
    out = []
    for col in itertools.product(*spans):
        ko = int(np.prod([cn for _, cn in col[:-1]], dtype=np.int64))
        st, cn = col[-1]
        out.append((ko * ((st + cn - 1) // v - st // v + 1), bpc))
    return out


def layer_rows(shape, chunks, index, axis):
    """``(reduced rows, first row's index along dim 0)`` of every chunk layer
    of a dense query: what k_trend_cols stages, ``kTrendRows`` a pass."""
    nd, P = len(shape), len(axis)
    index = per_dim(index, nd)
    spans = [_dim_spans(shape[d], chunks[d], index[d]) for d in range(P)]
    return [(int(np.prod([cn for _, cn in lay], dtype=np.int64)), lay[0][0]) for lay in itertools.product(*spans)]


def masked_selection(data, attrs, index):
    from pyactivestorage_amd.variable import get_missing_attributes
    return np.ma.asarray(ref.mask_missing(data[index], get_missing_attributes(attrs or {})))
