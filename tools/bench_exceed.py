"""Active.exceed on the resident C3 variable (1024^3 f32 in 64^3 chunks,
_FillValue + valid_min/valid_max, chunks attached in HBM), with its yardsticks
measured in the same run: argmax(0) and spell(0, "lt", t), whose dense kernels
issue the same loads, and mean(axis=(0,)), which reads the same bytes through
the dense fold.  Two exceed queries: "gt" a scalar t (the middle of the valid
range, as tools/bench_spell.py takes it) for the count, and "gt" a field of one
threshold per output (1 M points around t) for the sum.

Device chains (launch to stream synchronise, on prepared plans): exceed =
pyas_exceed_cols + pyas_exceed_finalize; argmax = pyas_argext_cols +
pyas_argext_finalize; spell = pyas_spell_cols + pyas_spell_finalize; mean =
pyas_reduce_axes_grid + pyas_format_partials.  Whole queries: the two exceed
queries, exceed with components, argmax, spell and mean, and the full
reduction exceed("gt", t)[...] beside var()[...].  Reported: exceed / argmax,
exceed / spell, exceed / mean and field / scalar for the device chain and the
whole query.  Median of --reps after warm-up, one process; the chains
alternate inside every repetition; two columns are checked against NumPy;
writes a JSON.

    python tools/bench_exceed.py [--reps 20] [--out profiles/exceed/bench_exceed.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.bench_argext import timed, timed_alternating  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "exceed", "bench_exceed.json"))
    a = ap.parse_args()
    import torch
    from pyactivestorage_amd import _lib, engine
    from pyactivestorage_amd.active import Active, attach_resident, release_resident
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer, get_context
    from pyactivestorage_amd.synthetic import chunk_major_device
    from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes
    cfg = bench.CONFIGS["c3"]
    dt = np.dtype(cfg["dtype"])
    shape, chunks = cfg["shape"], cfg["chunks"]
    dev = torch.device("cuda", 0)
    grid = [s // c for s, c in zip(shape, chunks)]
    cb = int(np.prod(chunks)) * dt.itemsize
    attrs = {"_FillValue": np.array([bench.FILL], dtype=dt), "valid_min": np.array([bench.VMIN], dtype=dt),
             "valid_max": np.array([bench.VMAX], dtype=dt)}
    data, offsets, _ = chunk_major_device(torch, shape, chunks, dt, dev, fill=bench.FILL, fill_frac=0.01, seed=0)
    index = {co: (int(offsets[k]), cb) for k, co in enumerate(np.ndindex(*grid))}
    var = ChunkedVariable(name="c3", shape=shape, chunks=chunks, dtype=dt, chunk_index=index, attrs=attrs,
                          filename=None, filter_pipeline=None)
    attach_resident(var, data.data_ptr(), device=0, owner=data)
    torch.cuda.synchronize()
    sync = torch.cuda.synchronize
    # the middle of the unmasked values 1000 .. 5e8, as tools/bench_spell.py takes it
    thr = float((int(bench.VMIN) + int(bench.VMAX)) // 2 + 16)
    # one threshold per output: the middle moved by up to +-2^20, another value at every point
    n_out = shape[1] * shape[2]
    field = (thr + ((np.arange(n_out, dtype=np.int64) * 2654435761 % (1 << 21)) - (1 << 20))
             ).astype(np.float64).reshape(1, shape[1], shape[2])
    res = {"workload": f"resident C3 variable {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       f"exceed('gt', {thr}, 'count', axis=(0,)) and exceed('gt', field, 'sum', axis=(0,)) against "
                       f"argmax(0), spell(0, 'lt', {thr}) and mean(axis=(0,)); exceed('gt', {thr})[...] against var()",
           "threshold": thr, "field_points": n_out, "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    comp = Active(var, resident=True)
    comp.components = True
    last = {}
    q = res["queries"]
    for name, fn in (("mean", lambda: act.mean(axis=(0,))[...]),
                     ("spell", lambda: act.spell(0, "lt", thr)[...]),
                     ("argmax", lambda: act.argmax(0)[...]),
                     ("exceed_count", lambda: act.exceed("gt", thr, "count", axis=(0,))[...]),
                     ("exceed_field_sum", lambda: act.exceed("gt", field, "sum", axis=(0,))[...]),
                     ("exceed_components", lambda: comp.exceed("gt", thr, axis=(0,))[...]),
                     ("var_full", lambda: act.var(axis=(0, 1, 2))[...]),
                     ("exceed_full", lambda: act.exceed("gt", thr, "count", axis=(0, 1, 2))[...])):
        def run(name=name, fn=fn):
            last[name] = fn()
        q[name + "_ms"], q[name + "_ms_min"] = timed(run, a.reps, sync)
        if name == "exceed_field_sum":
            q["exceed_path"] = act.exceed_path
        print(json.dumps({name: q[name + "_ms"]}), flush=True)
    for other in ("argmax", "spell", "mean"):
        q["exceed_count_over_" + other] = round(q["exceed_count_ms"] / q[other + "_ms"], 3)
    q["exceed_field_over_scalar"] = round(q["exceed_field_sum_ms"] / q["exceed_count_ms"], 3)
    q["exceed_full_over_var_full"] = round(q["exceed_full_ms"] / q["var_full_ms"], 3)
    q["result_shape"] = list(last["exceed_count"].shape)
    cnt, fsum = last["exceed_count"], last["exceed_field_sum"]
    res["result"] = {"masked_outputs": int(np.ma.getmaskarray(cnt).sum()),
                     "count_mean": round(float(cnt.mean()), 3), "full_count": int(last["exceed_full"].item())}
    # a spot check against NumPy: column (429, 238), which the scalar threshold cuts at row 133, and (1000, 300),
    # which lies above it
    col = data.view(torch.float32)
    spots = {}
    for j, k in ((429, 238), (1000, 300)):
        parts = []
        cj, ck = j // chunks[1], k // chunks[2]
        for l in range(grid[0]):
            o = int(offsets[(l * grid[1] + cj) * grid[2] + ck]) // 4
            parts.append(col[o:o + cb // 4].view(*chunks)[:, j % chunks[1], k % chunks[2]])
        y = torch.cat(parts).cpu().numpy().astype(np.float64)
        valid = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
        t = field[0, j, k]
        want_count = int((valid & (y > thr)).sum()) if valid.any() else -1
        want_sum = float(np.sum(y[valid & (y > t)])) if valid.any() else -1.0
        spots[f"{j},{k}"] = {"count": [int(cnt.filled(-1)[0, j, k]), want_count],
                             "field_sum": [float(fsum.filled(-1.0)[0, j, k]), want_sum]}
    res["spot_check"] = spots
    # the device chains on prepared plans
    ctx = get_context(0)
    st = ctx.thread_stream()
    n = int(np.prod(grid))
    plan = ReductionPlan(ctx, dt, chunks, data.data_ptr(), np.asarray(offsets, dtype=np.int64),
                         missing=get_missing_attributes(attrs), round_to_var=True, stream=st)
    g = _lib.Grid()
    g.ndim, g.axes_mask = 3, 1
    for d in range(3):
        g.n_coords[d] = grid[d]
        g.out_extent[d] = 1 if d == 0 else shape[d]
    coords = np.array(list(np.ndindex(*grid)), dtype=np.int64)
    origin32 = (coords[:, 0] * chunks[0]).astype(np.int32)
    fstride = np.array([0, shape[2], 1], dtype=np.int64)
    forigin = np.ascontiguousarray((coords * np.asarray(chunks, dtype=np.int64)) @ fstride, dtype=np.int64)
    obuf = DeviceBuffer(ctx, origin32.nbytes)
    ctx.h2d(obuf.ptr, origin32, st)
    fbuf = DeviceBuffer(ctx, field.nbytes + forigin.nbytes)
    ctx.h2d(fbuf.ptr, field, st)
    ctx.h2d(fbuf.ptr + field.nbytes, forigin, st)
    sfin = DeviceBuffer(ctx, n_out * _lib.SPELL_NBYTES)
    sval = DeviceBuffer(ctx, n_out * 5)
    afin = DeviceBuffer(ctx, n_out * _lib.ARGEXT_NBYTES)
    aval = DeviceBuffer(ctx, n_out * 5)
    efin = DeviceBuffer(ctx, n_out * _lib.EXCEED_NBYTES)
    evalue = DeviceBuffer(ctx, n_out * 9)
    pfin = DeviceBuffer(ctx, n_out * _lib.PARTIAL_NBYTES)
    mval, mmask = DeviceBuffer(ctx, n_out * 8), DeviceBuffer(ctx, n_out)
    ctx.synchronize(st)
    scalar_rule = engine.exceed_rule("gt", thr)
    field_rule = engine.exceed_rule("gt", 0.0, (fbuf.ptr, fbuf.ptr + field.nbytes, fstride))

    def exceed_chain(rule, stat):
        def chain():
            assert engine.exceed_cols(ctx, plan.batch, plan.mask_up.struct, rule, g, efin.ptr, st)
            engine.exceed_finalize(ctx, efin.ptr, n_out, stat, None, evalue.ptr, evalue.ptr + 8 * n_out, st)
            ctx.synchronize(st)
        return chain

    def exceed_kernel():
        assert engine.exceed_cols(ctx, plan.batch, plan.mask_up.struct, scalar_rule, g, efin.ptr, st)
        ctx.synchronize(st)

    def spell_chain():
        assert engine.spell_cols(ctx, plan.batch, plan.mask_up.struct, 0, "lt", thr, 1, g, sfin.ptr, st)
        engine.spell_finalize(ctx, sfin.ptr, n_out, "longest", sval.ptr, sval.ptr + 4 * n_out, st)
        ctx.synchronize(st)

    def argmax_chain():
        assert engine.argext_cols(ctx, plan.batch, plan.mask_up.struct, 0, "max", obuf.ptr, g, afin.ptr, st)
        engine.argext_finalize(ctx, afin.ptr, n_out, aval.ptr, aval.ptr + 4 * n_out, st)
        ctx.synchronize(st)

    def mean_chain():
        engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, pfin.ptr, True, st)
        engine.format_partials(ctx, dt, pfin.ptr, n_out, "mean", mval.ptr, mmask.ptr, None, st)
        ctx.synchronize(st)

    d = res["device_chain"] = {}
    got = timed_alternating({"exceed_count": exceed_chain(scalar_rule, "count"),
                             "exceed_field_sum": exceed_chain(field_rule, "sum"),
                             "argmax": argmax_chain, "spell": spell_chain, "mean": mean_chain,
                             "exceed_cols_only": exceed_kernel}, a.reps, sync)
    for name, (med, lo) in got.items():
        d[name + "_ms"], d[name + "_ms_min"] = med, lo
    for other in ("argmax", "spell", "mean"):
        d["exceed_count_over_" + other] = round(d["exceed_count_ms"] / d[other + "_ms"], 3)
        d["exceed_field_sum_over_" + other] = round(d["exceed_field_sum_ms"] / d[other + "_ms"], 3)
    d["exceed_field_over_scalar"] = round(d["exceed_field_sum_ms"] / d["exceed_count_ms"], 3)
    for name in ("exceed_count", "exceed_field_sum", "argmax", "spell", "mean"):
        d["GBps_" + name] = round(n * cb / d[name + "_ms"] / 1e6, 1)
    release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
