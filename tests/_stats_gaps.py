"""Shapes and data of the branch-coverage cases shared by the five statistics
modules (``test_gpu_moments``, ``test_gpu_weighted``, ``test_gpu_histogram``,
``test_gpu_quantile``, ``test_gpu_comoments``).  Each module runs these cases
through its own ``make_var`` / ``oracle`` / ``check`` / ``query``; nothing
here touches the device except :func:`misaligned_plan`.

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
"""
import functools

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

GROUPS = {"G1": G1, "G2": G2, "G3": G3, "G4": G4, "G5": G5}


def case(group, name):
    return GROUPS[group][name]


def combos(group, name):
    """Every ``(index name, index, axis, least valid elements per output)`` of a case."""
    shape, chunks, axes, indexes, _ = case(group, name)
    out = []
    for iname, index in indexes.items():
        for axis in axes:
            need = 2 if group in ("G2", "G4") else 0
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


def misaligned_plan(gpu, data, off, index=None):
    """``data`` as one chunk ``off`` bytes into a device buffer of exactly
    ``off + data.nbytes`` bytes, and the ReductionPlan of ``index`` (None: the
    whole chunk) over it: ``(stream, buffer, plan)``."""
    from pyactivestorage_amd import selection
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    st = gpu.thread_stream()
    host = np.zeros(off + data.nbytes, np.uint8)
    host[off:] = np.frombuffer(data.tobytes(), np.uint8)
    buf = DeviceBuffer(gpu, host.nbytes)
    assert buf.ptr % 16 == 0 and (buf.ptr + off) % 16 == off % 16 != 0
    gpu.h2d(buf.ptr, host, st)
    sels = None if index is None else [selection.normalize(index, data.shape)]
    plan = ReductionPlan(gpu, data.dtype, data.shape, buf.ptr, np.array([off], np.int64), selections=sels,
                         missing=(None,) * 4, stream=st)
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


def masked_selection(data, attrs, index):
    from pyactivestorage_amd.variable import get_missing_attributes
    return np.ma.asarray(ref.mask_missing(data[index], get_missing_attributes(attrs or {})))
