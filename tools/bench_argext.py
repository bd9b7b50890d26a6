"""Active.argmax(0) on the resident C3 variable (1024^3 f32 in 64^3 chunks,
_FillValue + valid_min/valid_max, chunks attached in HBM), with its three
yardsticks measured in the same run: spell(0, "lt", t), t the middle of the
valid range, and trend(0, axis=(0,)), whose dense kernels issue the same
loads, and mean(axis=(0,)), which reads the same bytes through the dense fold.

The variable's values grow by 1 per step along dim 0 (i + 1024 j + 1024^2 k),
so the maximum of a column is its last unmasked row and the accumulator is
replaced at every row.  It is updated by selects and takes no data-dependent
branch, so its time does not depend on where the extreme lies (argmin, whose
winner is the first unmasked row, is timed beside it).

Device chains (launch to stream synchronise, on prepared plans): argmax =
pyas_argext_cols + pyas_argext_finalize; spell = pyas_spell_cols +
pyas_spell_finalize; trend = pyas_trend_cols + pyas_trend_finalize; mean =
pyas_reduce_axes_grid + pyas_format_partials.  Whole queries: argmax, argmin,
argmax with components, spell, trend and mean.  Reported: argmax / spell,
argmax / trend and argmax / mean for the device chain and the whole query.
Median of --reps after warm-up, one process; the chains alternate inside every
repetition; writes a JSON.

    python tools/bench_argext.py [--reps 20] [--out profiles/argext/bench_argext.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def timed(fn, reps, sync):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        sync()
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return round(float(np.median(times)) * 1e3, 4), round(min(times) * 1e3, 4)


def timed_alternating(fns, reps, sync):
    """``{name: (median ms, min ms)}`` of several chains measured turn by
    turn, so that a drift of the machine meets all of them alike."""
    for fn in fns.values():
        for _ in range(3):
            fn()
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            sync()
            t0 = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t0)
    return {name: (round(float(np.median(t)) * 1e3, 4), round(min(t) * 1e3, 4)) for name, t in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "argext", "bench_argext.json"))
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
    # the middle of the unmasked values 1000 .. 5e8 (their median but for the fills), inside a column rather than
    # between two
    thr = float((int(bench.VMIN) + int(bench.VMAX)) // 2 + 16)
    res = {"workload": f"resident C3 variable {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       f"argmax(0) against spell(0, 'lt', {thr}), trend(0, axis=(0,)) and mean(axis=(0,))",
           "threshold": thr, "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    comp = Active(var, resident=True)
    comp.components = True
    last = {}
    q = res["queries"]
    for name, fn in (("mean", lambda: act.mean(axis=(0,))[...]),
                     ("trend", lambda: act.trend(0, axis=(0,))[...]),
                     ("spell", lambda: act.spell(0, "lt", thr)[...]),
                     ("argmax", lambda: act.argmax(0)[...]),
                     ("argmin", lambda: act.argmin(0)[...]),
                     ("argmax_components", lambda: comp.argmax(0)[...])):
        def run(name=name, fn=fn):
            last[name] = fn()
        q[name + "_ms"], q[name + "_ms_min"] = timed(run, a.reps, sync)
        print(json.dumps({name: q[name + "_ms"]}), flush=True)
    q["argext_path"] = act.argext_path
    for other in ("spell", "trend", "mean"):
        q["argmax_over_" + other] = round(q["argmax_ms"] / q[other + "_ms"], 3)
    q["result_shape"] = list(last["argmax"].shape)
    got, low = last["argmax"], last["argmin"]
    res["result"] = {"masked_outputs": int(np.ma.getmaskarray(got).sum()),
                     "argmax_mean": round(float(got.mean()), 2), "argmin_mean": round(float(low.mean()), 2)}
    # a spot check against NumPy: columns (5, 7) and (1000, 3)
    col = data.view(torch.float32)
    spots = {}
    for j, k in ((5, 7), (1000, 3)):
        parts = []
        cj, ck = j // chunks[1], k // chunks[2]
        for l in range(grid[0]):
            o = int(offsets[(l * grid[1] + cj) * grid[2] + ck]) // 4
            parts.append(col[o:o + cb // 4].view(*chunks)[:, j % chunks[1], k % chunks[2]])
        y = torch.cat(parts).cpu().numpy()
        valid = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
        live = np.nonzero(valid)[0]
        want = (int(live[np.argmax(y[live])]), int(live[np.argmin(y[live])])) if live.size else (-1, -1)
        spots[f"{j},{k}"] = {"got": [int(got.filled(-1)[0, j, k]), int(low.filled(-1)[0, j, k])], "want": list(want)}
    res["spot_check"] = spots
    # the device chains on prepared plans
    ctx = get_context(0)
    st = ctx.thread_stream()
    n = int(np.prod(grid))
    plan = ReductionPlan(ctx, dt, chunks, data.data_ptr(), np.asarray(offsets, dtype=np.int64),
                         missing=get_missing_attributes(attrs), round_to_var=True, stream=st)
    n_out = shape[1] * shape[2]
    g = _lib.Grid()
    g.ndim, g.axes_mask = 3, 1
    for d in range(3):
        g.n_coords[d] = grid[d]
        g.out_extent[d] = 1 if d == 0 else shape[d]
    cpool = np.arange(shape[0], dtype=np.float64)
    corigin = (np.array([co[0] for co in np.ndindex(*grid)], dtype=np.int64) * chunks[0]).astype(np.int32)
    cbuf = DeviceBuffer(ctx, cpool.nbytes + corigin.nbytes)
    ctx.h2d(cbuf.ptr, cpool, st)
    ctx.h2d(cbuf.ptr + cpool.nbytes, corigin, st)
    tfin = DeviceBuffer(ctx, n_out * _lib.COMOMENTS_NBYTES)
    tval = DeviceBuffer(ctx, n_out * 9)
    sfin = DeviceBuffer(ctx, n_out * _lib.SPELL_NBYTES)
    sval = DeviceBuffer(ctx, n_out * 5)
    afin = DeviceBuffer(ctx, n_out * _lib.ARGEXT_NBYTES)
    aval = DeviceBuffer(ctx, n_out * 5)
    pfin = DeviceBuffer(ctx, n_out * _lib.PARTIAL_NBYTES)
    mval, mmask = DeviceBuffer(ctx, n_out * 8), DeviceBuffer(ctx, n_out)
    ctx.synchronize(st)

    def spell_chain():
        assert engine.spell_cols(ctx, plan.batch, plan.mask_up.struct, 0, "lt", thr, 1, g, sfin.ptr, st)
        engine.spell_finalize(ctx, sfin.ptr, n_out, "longest", sval.ptr, sval.ptr + 4 * n_out, st)
        ctx.synchronize(st)

    origin = cbuf.ptr + cpool.nbytes   # the chunks' first rows: pyas_coord.origin and pyas_argext_rule.origin alike

    def argext_chain(which):
        def chain():
            assert engine.argext_cols(ctx, plan.batch, plan.mask_up.struct, 0, which, origin, g, afin.ptr, st)
            engine.argext_finalize(ctx, afin.ptr, n_out, aval.ptr, aval.ptr + 4 * n_out, st)
            ctx.synchronize(st)
        return chain

    def argmax_kernel():
        assert engine.argext_cols(ctx, plan.batch, plan.mask_up.struct, 0, "max", origin, g, afin.ptr, st)
        ctx.synchronize(st)

    def trend_chain():
        assert engine.trend_cols(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, 0, g,
                                 tfin.ptr, st)
        engine.trend_finalize(ctx, tfin.ptr, n_out, _lib.TREND_SLOPE, tval.ptr, tval.ptr + 8 * n_out, st)
        ctx.synchronize(st)

    def mean_chain():
        engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, pfin.ptr, True, st)
        engine.format_partials(ctx, dt, pfin.ptr, n_out, "mean", mval.ptr, mmask.ptr, None, st)
        ctx.synchronize(st)

    d = res["device_chain"] = {}
    got = timed_alternating({"mean": mean_chain, "trend": trend_chain, "spell": spell_chain,
                             "argmax": argext_chain("max"), "argmin": argext_chain("min"),
                             "argmax_cols_only": argmax_kernel}, a.reps, sync)
    for name, (med, lo) in got.items():
        d[name + "_ms"], d[name + "_ms_min"] = med, lo
    for other in ("spell", "trend", "mean"):
        d["argmax_over_" + other] = round(d["argmax_ms"] / d[other + "_ms"], 3)
    for name in ("argmax", "argmin", "spell", "trend", "mean"):
        d["GBps_" + name] = round(n * cb / d[name + "_ms"] / 1e6, 1)
    release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
