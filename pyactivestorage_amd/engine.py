"""Batch engine: drives the HIP kernels over chunks already in device memory.

This is the MI355X replacement for the reference's per-chunk loop
(``activestorage/active.py:557-598``): instead of one ``reduce_chunk`` call
per chunk on a 30-thread pool, one launch covers every chunk of a query.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from . import _lib
from .device import Context, DeviceBuffer
from .dtypes import dtype_code, native, needs_byteswap, sum_dtype, value_class
from .masking import CompiledMask, table_layout

_CLASS_DT = {"f": "<f8", "i": "<i8", "u": "<u8"}


def partial_dtype(dt) -> np.dtype:
    """Host view of ``pyas_partial`` for storage dtype dt."""
    c = _CLASS_DT[value_class(dt)]
    return np.dtype([("sum", c), ("count", "<i8"), ("min", c), ("max", c)])


# Host view of ``pyas_moments`` (every storage dtype: the record is f64)
moments_dtype = np.dtype([("count", "<i8"), ("mean", "<f8"), ("m2", "<f8"), ("reserved", "<u8")])
# Host view of ``pyas_comoments``
comoments_dtype = np.dtype([("count", "<i8"), ("mean_x", "<f8"), ("mean_y", "<f8"), ("m2_x", "<f8"),
                            ("m2_y", "<f8"), ("cxy", "<f8")])

# Host view of ``pyas_spell``
spell_dtype = np.dtype([(name, "<i4") for name in ("n", "n_true", "len", "head", "tail", "best", "days", "events",
                                                   "min_length", "reserved")])

# Host view of ``pyas_roll``
roll_dtype = np.dtype([("best", "<f8"), ("position", "<i4"), ("n_windows", "<i4"), ("n", "<i4"), ("len", "<i4"),
                       ("window", "u1"), ("which", "u1"), ("head_ok", "u1"), ("tail_ok", "u1"), ("reserved", "<i4"),
                       ("head", "<f8", (_lib.ROLL_MAX_WINDOW - 1,)), ("tail", "<f8", (_lib.ROLL_MAX_WINDOW - 1,))])

# Host view of ``pyas_argext``; ``value`` holds the bits of the pyas_scalar (view it as f8 / i8 / u8 by the
# data's class: :func:`pyactivestorage_amd.argext.values`)
argext_dtype = np.dtype([("value", "<u8"), ("index", "<i4"), ("n", "<i4")])

# Host view of ``pyas_exceed``
exceed_dtype = np.dtype([("n", "<i8"), ("n_true", "<i8"), ("sum", "<f8"), ("excess", "<f8")])

# Host view of ``pyas_wsum``
wsum_dtype = np.dtype([("count", "<i8"), ("sw", "<f8"), ("swx", "<f8"), ("reserved", "<u8")])

# Host view of ``pyas_wcomoments``
wcomoments_dtype = np.dtype([("count", "<i8"), ("sw", "<f8"), ("sw2", "<f8"), ("mean_x", "<f8"), ("mean_y", "<f8"),
                             ("m2_x", "<f8"), ("m2_y", "<f8"), ("cxy", "<f8")])


@dataclass
class Layout:
    """What every chunk of one variable shares."""
    dtype: np.dtype
    chunk_shape: tuple
    shuffle: int = 0          # fused HDF5 shuffle element size (0 = none)

    def batch_struct(self, n_chunks, data_ptr, offsets_ptr, sel_ptr=None, pool_ptr=None):
        b = _lib.Batch()
        b.dtype = dtype_code(self.dtype)
        b.byteswap = 1 if needs_byteswap(self.dtype) else 0
        b.shuffle = int(self.shuffle)
        b.ndim = len(self.chunk_shape)
        if not 1 <= b.ndim <= _lib.MAX_DIMS:
            raise NotImplementedError(f"chunk rank {b.ndim} outside 1..{_lib.MAX_DIMS}")
        for d, n in enumerate(self.chunk_shape):
            b.chunk_shape[d] = int(n)
        b.n_chunks = int(n_chunks)
        b.data = data_ptr
        b.offsets = offsets_ptr
        b.sel = sel_ptr
        b.index_pool = pool_ptr
        return b


class MaskUpload:
    """Device copy of a CompiledMask's vector tables for one selected shape."""

    def __init__(self, ctx: Context, cm: CompiledMask, sel_shape, kept, stream):
        self.struct = cm.to_struct()
        self._bufs = []
        for k, which in ((0, "_FillValue"), (1, "missing_value")):
            if cm.tables[k] is None:
                continue
            strides = table_layout(cm, k, sel_shape, "missing_value" if k == 1 else "fill")
            lo, hi, _ = cm.tables[k]
            nd = native(cm.dt)
            host = np.zeros((2, lo.size), dtype=_CLASS_DT[value_class(nd)])
            host[0] = lo
            host[1] = hi
            buf = DeviceBuffer(ctx, host.nbytes)
            ctx.h2d(buf.ptr, host, stream)
            self._bufs.append(buf)
            self.struct.tab_len[k] = lo.size
            self.struct.tab_lo[k] = buf.ptr
            self.struct.tab_hi[k] = buf.ptr + lo.size * 8
            for j, d in enumerate(kept):
                self.struct.tab_stride[k][d] = int(strides[j])

    def keepalive(self):
        return self._bufs


def reduce_chunks(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, chunk_out_ptr, total_ptr,
                  round_to_var: bool, stream) -> None:
    flags = _lib.COMBINE_ROUND_TO_VAR if round_to_var else 0
    _lib.check(ctx.lib.pyas_reduce_chunks(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                          chunk_out_ptr, total_ptr, flags, stream),
               "pyas_reduce_chunks")


def tie_chunks(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, geom: _lib.TieGeom, axes_mask: int,
               which: int, out_offsets_ptr, partials_ptr, stream) -> None:
    """NumPy's sign of every zero min (which 1) / max (which 2) among the
    chunks' partials (pyas_tie_chunks, storage.py:99-100)."""
    _lib.check(ctx.lib.pyas_tie_chunks(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(geom),
                                       int(axes_mask), int(which), out_offsets_ptr, partials_ptr, stream),
               "pyas_tie_chunks")


def tie_chunks_total(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, geom: _lib.TieGeom, which: int,
                     partials_ptr, layer_base: int, lr: int, stream) -> None:
    """Level 1 of a full reduction where it can matter (pyas_tie_chunks_total):
    only the two chunks the level-2 keys can pick are scanned, so
    tie_segments afterwards gives what tie_chunks over every chunk would."""
    _lib.check(ctx.lib.pyas_tie_chunks_total(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                             ctypes.byref(geom), int(which), partials_ptr, int(layer_base),
                                             int(lr), stream),
               "pyas_tie_chunks_total")


def tie_chunk_flags(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, geom: _lib.TieGeom, axes_mask: int,
                    which: int, out_offsets_ptr, final_ptr, n_final: int, flags_ptr, stream) -> None:
    """Per chunk output: zero held / NumPy's sign, when a final min/max is a
    zero (pyas_tie_chunk_flags; for results folded in the reduce kernel)."""
    _lib.check(ctx.lib.pyas_tie_chunk_flags(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                            ctypes.byref(geom), int(axes_mask), int(which), out_offsets_ptr,
                                            final_ptr, int(n_final), flags_ptr, stream),
               "pyas_tie_chunk_flags")


def tie_grid(ctx: Context, dt, grid: _lib.Grid, parts_ptr, flags_ptr, lr: int, which: int, final_ptr,
             keys_ptr, stream) -> None:
    """NumPy's sign of the zero min/max of the `out` reduction over chunk
    layers (pyas_tie_grid, active.py:594)."""
    _lib.check(ctx.lib.pyas_tie_grid(ctx.handle, dtype_code(dt), ctypes.byref(grid), parts_ptr, flags_ptr,
                                     int(lr), int(which), final_ptr, keys_ptr, stream), "pyas_tie_grid")


def tie_segments(ctx: Context, dt, parts_ptr, index_ptr, seg_ptr, n_seg: int, n_layers: int, layer_base: int,
                 lr: int, which: int, final_ptr, keys_ptr, stream) -> None:
    """pyas_tie_segments: the level-2 sign over segment lists (or one
    output over parts[0, n_layers) when index/seg are None)."""
    _lib.check(ctx.lib.pyas_tie_segments(ctx.handle, dtype_code(dt), parts_ptr, index_ptr, seg_ptr, int(n_seg),
                                         int(n_layers), int(layer_base), int(lr), int(which), final_ptr,
                                         keys_ptr, stream), "pyas_tie_segments")


def tie_keys_reset(ctx: Context, keys_ptr, n_out: int, stream) -> None:
    _lib.check(ctx.lib.pyas_tie_keys_reset(ctx.handle, keys_ptr, int(n_out), stream), "pyas_tie_keys_reset")


def tie_finalize(ctx: Context, dt, keys_ptr, n_out: int, n_sets: int, lr: int, which: int, final_ptr,
                 stream) -> None:
    """Combine gathered keys (ranks) and write the signs (pyas_tie_finalize)."""
    _lib.check(ctx.lib.pyas_tie_finalize(ctx.handle, dtype_code(dt), keys_ptr, int(n_out), int(n_sets), int(lr),
                                         int(which), final_ptr, stream), "pyas_tie_finalize")


def reduce_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, axes_mask: int, out_offsets_ptr,
                out_ptr, stream, rec: int = 0) -> None:
    """pyas_reduce_axes, or with ``rec`` (PYAS_REC_SUM/MIN/MAX) the compact
    per-output records of pyas_reduce_axes_ex."""
    _lib.check(ctx.lib.pyas_reduce_axes_ex(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                           int(axes_mask), int(rec), out_offsets_ptr, out_ptr, stream),
               "pyas_reduce_axes_ex")


def method_rec(method) -> int:
    """The record form a partial-axis query of ``method`` needs per chunk
    output (storage.py:98-100): the rounded sum for sum/mean, else the min
    or the max."""
    return {"min": _lib.REC_MIN, "max": _lib.REC_MAX}.get(method, _lib.REC_SUM)


def reduce_axes_grid(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, grid: _lib.Grid, out_ptr,
                     round_to_var: bool, stream, zero_sign: int = 0) -> None:
    """pyas_reduce_axes + pyas_combine_grid in one launch (whole chunks);
    NotImplementedError when the geometry does not admit it.  ``zero_sign``
    (1 min, 2 max): NumPy's sign of a zero result fused into the fold
    (PYAS_FOLD_ZERO_SIGN_*; the caller checks both reductions are
    elementwise)."""
    flags = (_lib.COMBINE_ROUND_TO_VAR if round_to_var else 0) | (int(zero_sign) << 8)
    _lib.check(ctx.lib.pyas_reduce_axes_grid(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                             ctypes.byref(grid), flags, out_ptr, stream),
               "pyas_reduce_axes_grid")


def select_chunks(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, out_offsets_ptr, values_ptr,
                  mask_out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_select_chunks(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                          out_offsets_ptr, values_ptr, mask_out_ptr, stream),
               "pyas_select_chunks")


def select_scatter(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, scatter: _lib.Scatter,
                   values_ptr, mask_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_select_scatter(ctx.handle, ctypes.byref(batch), ctypes.byref(mask),
                                           ctypes.byref(scatter), values_ptr, mask_ptr, stream),
               "pyas_select_scatter")


def combine_partials(ctx: Context, dt, in_ptr, n, out_ptr, round_to_var: bool, stream) -> None:
    flags = _lib.COMBINE_ROUND_TO_VAR if round_to_var else 0
    _lib.check(ctx.lib.pyas_combine_partials(ctx.handle, dtype_code(dt), in_ptr, int(n), flags,
                                             out_ptr, stream), "pyas_combine_partials")


def combine_segments(ctx: Context, dt, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, round_to_var: bool,
                     stream, rec: int = 0) -> None:
    flags = (_lib.COMBINE_ROUND_TO_VAR if round_to_var else 0) | _lib.combine_rec(rec)
    _lib.check(ctx.lib.pyas_combine_segments(ctx.handle, dtype_code(dt), in_ptr, index_ptr, seg_ptr,
                                             int(n_seg), flags, out_ptr, stream),
               "pyas_combine_segments")


def combine_grid(ctx: Context, dt, in_ptr, grid: _lib.Grid, out_ptr, round_to_var: bool, stream,
                 rec: int = 0, zero_sign: int = 0) -> None:
    """pyas_combine_grid.  ``zero_sign`` (1 min, 2 max): the records carry
    level 1's NumPy sign (PYAS_REC_ZERO_SIGN) and the combine keys level 2
    (PYAS_FOLD_ZERO_SIGN_*) over the `out` array's calls."""
    flags = (_lib.COMBINE_ROUND_TO_VAR if round_to_var else 0) | _lib.combine_rec(rec) | (int(zero_sign) << 8)
    _lib.check(ctx.lib.pyas_combine_grid(ctx.handle, dtype_code(dt), in_ptr, ctypes.byref(grid), flags,
                                         out_ptr, stream), "pyas_combine_grid")


def moments_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, axes_mask: int, out_offsets_ptr, out_ptr,
                 stream) -> None:
    """pyas_moments_axes: count / mean / m2 records per chunk output (one per
    chunk, at ``out[c]`` when ``out_offsets_ptr`` is None, with every dim in
    ``axes_mask``)."""
    _lib.check(ctx.lib.pyas_moments_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), int(axes_mask),
                                         out_offsets_ptr, out_ptr, stream), "pyas_moments_axes")


def moments_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_moments_combine_segments (``index_ptr`` None: the identity)."""
    _lib.check(ctx.lib.pyas_moments_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                     stream), "pyas_moments_combine_segments")


def moments_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_moments_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_moments_combine_grid")


def comoments_axes(ctx: Context, batch_x: _lib.Batch, mask_x: _lib.Mask, batch_y: _lib.Batch, mask_y: _lib.Mask,
                   axes_mask: int, out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_comoments_axes: count / means / m2s / cxy records per chunk output
    of the pairs of two variables (chunk c of ``batch_y`` against chunk c of
    ``batch_x``, under ``batch_x``'s selection); outputs as :func:`moments_axes`'."""
    _lib.check(ctx.lib.pyas_comoments_axes(ctx.handle, ctypes.byref(batch_x), ctypes.byref(mask_x),
                                           ctypes.byref(batch_y), ctypes.byref(mask_y), int(axes_mask),
                                           out_offsets_ptr, out_ptr, stream), "pyas_comoments_axes")


def comoments_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_comoments_combine_segments (``index_ptr`` None: the identity)."""
    _lib.check(ctx.lib.pyas_comoments_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                       stream), "pyas_comoments_combine_segments")


def comoments_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_comoments_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_comoments_combine_grid")


def trend_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, pool_ptr, origin_ptr, dim: int, axes_mask: int,
               out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_trend_axes: co-moment records of the data against a coordinate per
    chunk output, laid out like :func:`moments_axes`'; ``pool_ptr`` /
    ``origin_ptr`` / ``dim``: pyas_coord."""
    c = _lib.Coord(pool_ptr, origin_ptr, int(dim))
    _lib.check(ctx.lib.pyas_trend_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(c),
                                       int(axes_mask), out_offsets_ptr, out_ptr, stream), "pyas_trend_axes")


def trend_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, pool_ptr, origin_ptr, dim: int, grid: _lib.Grid,
               out_ptr, stream) -> bool:
    """pyas_trend_cols: one finished record per final output of a unit-step
    box query, in one launch.  False (nothing launched) when the geometry is
    not the dense path's (PYAS_ENOTSUP): the caller runs :func:`trend_axes`."""
    c = _lib.Coord(pool_ptr, origin_ptr, int(dim))
    rc = ctx.lib.pyas_trend_cols(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(c),
                                 ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, "pyas_trend_cols")
    return True


def trend_finalize(ctx: Context, in_ptr, n: int, what: int, value_ptr, mask_ptr, stream) -> None:
    """pyas_trend_finalize: slope (``_lib.TREND_SLOPE``) or intercept of ``n``
    records as float64 values and mask bytes, on the device."""
    _lib.check(ctx.lib.pyas_trend_finalize(ctx.handle, in_ptr, int(n), int(what), value_ptr, mask_ptr, stream),
               "pyas_trend_finalize")


def _spell_rule(dim: int, op: str, threshold: float, min_length: int) -> _lib.SpellRule:
    return _lib.SpellRule(int(dim), _lib.SPELL_OPS[op], int(min_length), float(threshold))


def spell_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, op: str, threshold: float,
               min_length: int, out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_spell_axes: spell records along chunk dim ``dim`` (the one reduced
    dim) per chunk output, laid out like :func:`moments_axes`'."""
    rule = _spell_rule(dim, op, threshold, min_length)
    _lib.check(ctx.lib.pyas_spell_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                       1 << int(dim), out_offsets_ptr, out_ptr, stream), "pyas_spell_axes")


def spell_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, op: str, threshold: float,
               min_length: int, grid: _lib.Grid, out_ptr, stream) -> bool:
    """pyas_spell_cols: one finished record per final output of a unit-step
    box query, in one launch.  False (nothing launched) when the geometry is
    not the dense path's (PYAS_ENOTSUP): the caller runs :func:`spell_axes`."""
    rule = _spell_rule(dim, op, threshold, min_length)
    rc = ctx.lib.pyas_spell_cols(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                 ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, "pyas_spell_cols")
    return True


def spell_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_spell_combine_segments (``index_ptr`` None: the identity); the
    records of a segment in sequence order."""
    _lib.check(ctx.lib.pyas_spell_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                   stream), "pyas_spell_combine_segments")


def spell_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_spell_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_spell_combine_grid")


def spell_finalize(ctx: Context, in_ptr, n: int, stat: str, value_ptr, mask_ptr, stream) -> None:
    """pyas_spell_finalize: ``stat`` (``longest``, ``days`` or ``events``) of
    ``n`` records as int32 values and mask bytes, on the device."""
    _lib.check(ctx.lib.pyas_spell_finalize(ctx.handle, in_ptr, int(n), _lib.SPELL_STATS[stat], value_ptr, mask_ptr,
                                           stream), "pyas_spell_finalize")


def _roll_rule(dim: int, window: int, which: str) -> _lib.RollRule:
    return _lib.RollRule(int(dim), int(window), _lib.ROLL_WHICH[which])


def roll_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, window: int, which: str,
              out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_roll_axes: running-window records along chunk dim ``dim`` (the one
    reduced dim); ``out_offsets_ptr`` None for a 1-D variable."""
    rule = _roll_rule(dim, window, which)
    _lib.check(ctx.lib.pyas_roll_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                      1 << int(dim), out_offsets_ptr, out_ptr, stream), "pyas_roll_axes")


def roll_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, window: int, which: str,
              grid: _lib.Grid, out_ptr, stream) -> bool:
    """pyas_roll_cols: one finished record per final output of a unit-step
    box query with dim 0 the one reduced dim.  False when the geometry is
    not the dense path's (PYAS_ENOTSUP): the caller runs :func:`roll_axes`."""
    rule = _roll_rule(dim, window, which)
    rc = ctx.lib.pyas_roll_cols(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, "pyas_roll_cols")
    return True


def roll_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_roll_combine_segments (``index_ptr`` None: the identity); the
    records of a segment are listed in sequence order."""
    _lib.check(ctx.lib.pyas_roll_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                  stream), "pyas_roll_combine_segments")


def roll_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_roll_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_roll_combine_grid")


def roll_finalize(ctx: Context, in_ptr, n: int, stat: str, value_ptr, mask_ptr, stream) -> None:
    """pyas_roll_finalize: ``stat`` (``sum`` or ``mean``) of ``n`` records as
    float64 and the mask bytes, on the device."""
    _lib.check(ctx.lib.pyas_roll_finalize(ctx.handle, in_ptr, int(n), _lib.ROLL_STATS[stat], value_ptr, mask_ptr,
                                          stream), "pyas_roll_finalize")


def _argext_rule(dim: int, which: str, origin_ptr) -> _lib.ArgextRule:
    return _lib.ArgextRule(int(dim), _lib.ARGEXT_WHICH[which], origin_ptr)


def argext_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, which: str, origin_ptr,
                out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_argext_axes: arg-extreme records (``which``: ``max`` or ``min``)
    along chunk dim ``dim`` (the one reduced dim) per chunk output, laid out
    like :func:`moments_axes`'; ``origin_ptr``: each chunk's global index 0
    along ``dim`` (device int32)."""
    rule = _argext_rule(dim, which, origin_ptr)
    _lib.check(ctx.lib.pyas_argext_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                        1 << int(dim), out_offsets_ptr, out_ptr, stream), "pyas_argext_axes")


def argext_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, dim: int, which: str, origin_ptr,
                grid: _lib.Grid, out_ptr, stream) -> bool:
    """pyas_argext_cols: one finished record per final output of a unit-step
    box query, in one launch.  False (nothing launched) when the geometry is
    not the dense path's (PYAS_ENOTSUP): the caller runs :func:`argext_axes`."""
    rule = _argext_rule(dim, which, origin_ptr)
    rc = ctx.lib.pyas_argext_cols(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                  ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, "pyas_argext_cols")
    return True


def argext_combine_segments(ctx: Context, dt, which: str, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr,
                            stream) -> None:
    """pyas_argext_combine_segments (``index_ptr`` None: the identity) for
    records of data of dtype ``dt``."""
    _lib.check(ctx.lib.pyas_argext_combine_segments(ctx.handle, dtype_code(dt), _lib.ARGEXT_WHICH[which], in_ptr,
                                                    index_ptr, seg_ptr, int(n_seg), out_ptr, stream),
               "pyas_argext_combine_segments")


def argext_combine_grid(ctx: Context, dt, which: str, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_argext_combine_grid(ctx.handle, dtype_code(dt), _lib.ARGEXT_WHICH[which], in_ptr,
                                                ctypes.byref(grid), out_ptr, stream), "pyas_argext_combine_grid")


def argext_finalize(ctx: Context, in_ptr, n: int, index_ptr, mask_ptr, stream) -> None:
    """pyas_argext_finalize: the global index of ``n`` records as int32 and
    the mask bytes, on the device."""
    _lib.check(ctx.lib.pyas_argext_finalize(ctx.handle, in_ptr, int(n), index_ptr, mask_ptr, stream),
               "pyas_argext_finalize")


def exceed_rule(op: str, threshold: float, field=None) -> _lib.ExceedRule:
    """pyas_exceed_rule for a scalar ``threshold``, or for a per-output field
    ``(values_ptr, origin_ptr, strides)`` (device pointers; one element stride
    per dim, 0 on reduced dims).  The returned struct keeps the field struct
    alive (``rule.field_struct``)."""
    if field is None:
        return _lib.ExceedRule(_lib.SPELL_OPS[op], 0, float(threshold), None)
    values_ptr, origin_ptr, strides = field
    f = _lib.ExceedField(values_ptr, origin_ptr, (ctypes.c_int64 * _lib.MAX_DIMS)(*[int(s) for s in strides]))
    rule = _lib.ExceedRule(_lib.SPELL_OPS[op], 0, 0.0, ctypes.pointer(f))
    rule.field_struct = f
    return rule


def exceed_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, rule: _lib.ExceedRule, axes_mask: int,
                out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_exceed_axes: exceed records over the dims of ``axes_mask`` per
    chunk output, laid out like :func:`moments_axes`' (``out_offsets_ptr`` may
    be None only when every dim is reduced)."""
    _lib.check(ctx.lib.pyas_exceed_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                        int(axes_mask), out_offsets_ptr, out_ptr, stream), "pyas_exceed_axes")


def exceed_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, rule: _lib.ExceedRule, grid: _lib.Grid, out_ptr,
                stream) -> bool:
    """pyas_exceed_cols: one finished record per final output of a unit-step
    box query, in one launch.  False (nothing launched) when the geometry is
    not the dense path's (PYAS_ENOTSUP): the caller runs :func:`exceed_axes`."""
    rc = ctx.lib.pyas_exceed_cols(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rule),
                                  ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, "pyas_exceed_cols")
    return True


def exceed_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_exceed_combine_segments (``index_ptr`` None: the identity)."""
    _lib.check(ctx.lib.pyas_exceed_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                    stream), "pyas_exceed_combine_segments")


def exceed_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_exceed_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_exceed_combine_grid")


def exceed_finalize(ctx: Context, in_ptr, n: int, stat: str, thr_masked_ptr, value_ptr, mask_ptr, stream) -> None:
    """pyas_exceed_finalize: ``stat`` of ``n`` records (8 bytes each: int64
    for ``count``, float64 otherwise) and the mask bytes, on the device;
    ``thr_masked_ptr``: one byte per output, non-zero where its threshold is
    masked, or None."""
    _lib.check(ctx.lib.pyas_exceed_finalize(ctx.handle, in_ptr, int(n), _lib.EXCEED_STATS[stat], thr_masked_ptr,
                                            value_ptr, mask_ptr, stream), "pyas_exceed_finalize")


def group_cols(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, layer_ptr, offset_ptr, label_ptr, n_rows: int,
               n_groups: int, grid: _lib.Grid, out_ptr, stream, partial: bool = False) -> bool:
    """pyas_group_cols: one finished moments record per (group, final output)
    of a unit-step box query, in one launch, over the sorted row list
    (``grouped.row_list``).  False (nothing launched) when the geometry is not
    the dense path's (PYAS_ENOTSUP): the caller runs :func:`group_axes`.
    ``partial``: pyas_group_cols_partial, the same over ``partial_dtype``
    records."""
    name = "pyas_group_cols_partial" if partial else "pyas_group_cols"
    rows = _lib.GroupRows(layer_ptr, offset_ptr, label_ptr, int(n_rows), int(n_groups))
    rc = getattr(ctx.lib, name)(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(rows),
                                ctypes.byref(grid), out_ptr, stream)
    if rc == _lib.ENOTSUP:
        return False
    _lib.check(rc, name)
    return True


def group_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, start_ptr, ptr_ptr, pos_ptr, dim: int,
               axes_mask: int, out_offsets_ptr, out_ptr, stream, partial: bool = False) -> None:
    """pyas_group_axes: moments records per (chunk output, chunk-local group);
    ``start_ptr`` / ``ptr_ptr`` / ``pos_ptr`` / ``dim``: pyas_group_lists
    (``grouped.chunk_lists``).  ``partial``: pyas_group_axes_partial, the same
    over ``partial_dtype`` records."""
    name = "pyas_group_axes_partial" if partial else "pyas_group_axes"
    lists = _lib.GroupLists(start_ptr, ptr_ptr, pos_ptr, int(dim))
    _lib.check(getattr(ctx.lib, name)(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(lists),
                                      int(axes_mask), out_offsets_ptr, out_ptr, stream), name)


def hist_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, edges_ptr, n_bins: int, uniform, axes_mask: int,
              out_offsets_ptr, out_index_ptr, table_ptr, stream) -> None:
    """pyas_hist_axes: binned counts added into int64 table rows of
    ``n_bins + 3`` slots (counts, below, above, nan).  ``edges_ptr``: the
    ``n_bins + 1`` float64 edges on the device; ``uniform``: None, or the
    ``(lo, scale)`` of the kernels' first guess for evenly spaced edges.
    ``out_offsets_ptr`` may be None with every dim in ``axes_mask`` (row 0);
    ``out_index_ptr`` None is the identity."""
    h = _lib.Hist(edges_ptr, int(n_bins), 0, 0.0, 0.0)
    if uniform is not None:
        h.flags, h.lo, h.scale = _lib.HIST_UNIFORM, float(uniform[0]), float(uniform[1])
    _lib.check(ctx.lib.pyas_hist_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(h),
                                      int(axes_mask), out_offsets_ptr, out_index_ptr, table_ptr, stream),
               "pyas_hist_axes")


def hist_reset(ctx: Context, table_ptr, n_rows: int, n_bins: int, stream) -> None:
    """pyas_hist_reset: zero ``n_rows`` table rows on the stream."""
    _lib.check(ctx.lib.pyas_hist_reset(ctx.handle, table_ptr, int(n_rows), int(n_bins), stream), "pyas_hist_reset")


def select_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, prefix_ptr, shift: int, bits: int, axes_mask: int,
                out_offsets_ptr, out_index_ptr, table_ptr, stream) -> None:
    """pyas_select_axes: one pass of the radix select, the counts of the digit
    of ``bits`` bits at ``shift`` added into int64 table rows of
    ``2^bits + 3`` slots (digit counts, below, above, nan).  ``prefix_ptr``:
    the device uint64 prefixes, one per row (None on the first pass); the
    other arguments as for :func:`hist_axes`."""
    s = _lib.Select(prefix_ptr, int(shift), int(bits))
    _lib.check(ctx.lib.pyas_select_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(s),
                                        int(axes_mask), out_offsets_ptr, out_index_ptr, table_ptr, stream),
               "pyas_select_axes")


def select_step(ctx: Context, table_ptr, n_rows: int, bits: int, rank_ptr, prefix_ptr, below_base_ptr,
                stream) -> None:
    """pyas_select_step: extend every row's prefix by the digit that holds
    its rank (all pointers device; ``below_base_ptr`` may be None)."""
    _lib.check(ctx.lib.pyas_select_step(ctx.handle, table_ptr, int(n_rows), int(bits), rank_ptr, prefix_ptr,
                                        below_base_ptr, stream), "pyas_select_step")


def select_totals(ctx: Context, table_ptr, n_rows: int, bits: int, totals_ptr, stream) -> None:
    """pyas_select_totals: ``(n, nan)`` int64 per table row, on the device."""
    _lib.check(ctx.lib.pyas_select_totals(ctx.handle, table_ptr, int(n_rows), int(bits), totals_ptr, stream),
               "pyas_select_totals")


def wsum_axes(ctx: Context, batch: _lib.Batch, mask: _lib.Mask, pool_ptr, origin_ptr, axes_mask: int,
              out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_wsum_axes: count / sum w / sum w x records per chunk output, laid
    out like :func:`moments_axes`'; ``pool_ptr`` / ``origin_ptr``: pyas_weights."""
    w = _lib.Weights(pool_ptr, origin_ptr)
    _lib.check(ctx.lib.pyas_wsum_axes(ctx.handle, ctypes.byref(batch), ctypes.byref(mask), ctypes.byref(w),
                                      int(axes_mask), out_offsets_ptr, out_ptr, stream), "pyas_wsum_axes")


def wsum_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_wsum_combine_segments (``index_ptr`` None: the identity)."""
    _lib.check(ctx.lib.pyas_wsum_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                  stream), "pyas_wsum_combine_segments")


def wsum_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_wsum_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_wsum_combine_grid")


def wcomoments_axes(ctx: Context, batch_x: _lib.Batch, mask_x: _lib.Mask, batch_y, mask_y, pool_ptr, origin_ptr,
                    axes_mask: int, out_offsets_ptr, out_ptr, stream) -> None:
    """pyas_wcomoments_axes: count / sw / sw2 / means / m2s / cxy records per
    chunk output, laid out like :func:`moments_axes`'; ``batch_y`` None: one
    variable (``mask_y`` ignored); ``pool_ptr`` / ``origin_ptr``: pyas_weights."""
    w = _lib.Weights(pool_ptr, origin_ptr)
    by = ctypes.byref(batch_y) if batch_y is not None else None
    my = ctypes.byref(mask_y) if batch_y is not None else None
    _lib.check(ctx.lib.pyas_wcomoments_axes(ctx.handle, ctypes.byref(batch_x), ctypes.byref(mask_x), by, my,
                                            ctypes.byref(w), int(axes_mask), out_offsets_ptr, out_ptr, stream),
               "pyas_wcomoments_axes")


def wcomoments_combine_segments(ctx: Context, in_ptr, index_ptr, seg_ptr, n_seg, out_ptr, stream) -> None:
    """pyas_wcomoments_combine_segments (``index_ptr`` None: the identity)."""
    _lib.check(ctx.lib.pyas_wcomoments_combine_segments(ctx.handle, in_ptr, index_ptr, seg_ptr, int(n_seg), out_ptr,
                                                        stream), "pyas_wcomoments_combine_segments")


def wcomoments_combine_grid(ctx: Context, in_ptr, grid: _lib.Grid, out_ptr, stream) -> None:
    _lib.check(ctx.lib.pyas_wcomoments_combine_grid(ctx.handle, in_ptr, ctypes.byref(grid), out_ptr, stream),
               "pyas_wcomoments_combine_grid")


_FORMAT = {"sum": _lib.FORMAT_SUM, "min": _lib.FORMAT_MIN, "max": _lib.FORMAT_MAX,
           "mean": _lib.FORMAT_MEAN}


def format_dtype(dt, method: str) -> np.dtype:
    """Element type pyas_format_partials writes for ``method``."""
    if method == "mean":
        return np.dtype(np.float64)
    if method == "sum":
        return native(dt) if np.dtype(dt).kind == "f" else sum_dtype(dt)
    return native(dt)


def format_partials(ctx: Context, dt, in_ptr, n, method: str, values_ptr, mask_ptr, counts_ptr,
                    stream) -> None:
    """Device form of ``Active._format`` (active.py:591-630) over n partials."""
    _lib.check(ctx.lib.pyas_format_partials(ctx.handle, dtype_code(dt), in_ptr, int(n), _FORMAT[method],
                                            values_ptr, mask_ptr, counts_ptr, stream),
               "pyas_format_partials")


def unshuffle(ctx: Context, src_ptr, dst_ptr, nbytes, elementsize, stream) -> None:
    _lib.check(ctx.lib.pyas_unshuffle(ctx.handle, src_ptr, dst_ptr, int(nbytes), int(elementsize),
                                      stream), "pyas_unshuffle")


def unshuffle_chunks(ctx: Context, src_ptr, src_offsets_ptr, dst_ptr, dst_offsets_ptr, n_chunks,
                     chunk_bytes, elementsize, stream) -> None:
    """Batched device un-shuffle of whole chunks (offset arrays on the device)."""
    _lib.check(ctx.lib.pyas_unshuffle_chunks(ctx.handle, src_ptr, src_offsets_ptr, dst_ptr, dst_offsets_ptr,
                                             int(n_chunks), int(chunk_bytes), int(elementsize), stream),
               "pyas_unshuffle_chunks")
