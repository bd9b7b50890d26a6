"""Active.rolling(0, 5) (Rx5day) on the resident C3 variable (1024^3 f32 in
64^3 chunks, _FillValue + valid_min/valid_max, chunks attached in HBM), with
its yardsticks measured in the same run: trend(0, axis=(0,)), whose dense
kernel issues the same loads and does comparable float64 work per element,
spell(0, "lt", t), and mean(axis=(0,)), which reads the same bytes through the
dense fold.

The variable's values grow by 1 per step along dim 0, so the largest window of
a column is its last valid one; the 1 % of planted fill values remove 5 windows
each.  The kernel's accumulator takes no data-dependent branch, so its time
does not depend on where the extreme lies.

Device chains (launch to stream synchronise, on prepared plans): rolling =
pyas_roll_cols + pyas_roll_finalize for w = 5 (and w = 1, 3, 8); trend =
pyas_trend_cols + pyas_trend_finalize; spell = pyas_spell_cols +
pyas_spell_finalize; mean = pyas_reduce_axes_grid + pyas_format_partials.
Whole queries: rolling (sum, w = 5), rolling with components, trend, spell and
mean.  Reported: rolling / trend for the device chain and the whole query.
Median of --reps after warm-up, one process; the chains alternate inside every
repetition; writes a JSON.

    python tools/bench_rolling.py [--reps 20] [--out profiles/rolling/bench_rolling.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

WINDOWS = (5, 1, 3, 8)


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
    ap.add_argument("--out", default=os.path.join("profiles", "rolling", "bench_rolling.json"))
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
    thr = float((int(bench.VMIN) + int(bench.VMAX)) // 2 + 16)   # the spell yardstick's threshold (tools/bench_spell.py)
    res = {"workload": f"resident C3 variable {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       f"rolling(0, 5) against trend(0, axis=(0,)), spell(0, 'lt', {thr}) and mean(axis=(0,))",
           "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    comp = Active(var, resident=True)
    comp.components = True
    last = {}
    q = res["queries"]
    for name, fn in (("mean", lambda: act.mean(axis=(0,))[...]),
                     ("trend", lambda: act.trend(0, axis=(0,))[...]),
                     ("spell", lambda: act.spell(0, "lt", thr)[...]),
                     ("rolling_w5", lambda: act.rolling(0, 5)[...]),
                     ("rolling_w5_mean_min", lambda: act.rolling(0, 5, stat="mean", extreme="min")[...]),
                     ("rolling_w5_components", lambda: comp.rolling(0, 5)[...])):
        def run(name=name, fn=fn):
            last[name] = fn()
        q[name + "_ms"], q[name + "_ms_min"] = timed(run, a.reps, sync)
        print(json.dumps({name: q[name + "_ms"]}), flush=True)
    q["rolling_path"] = act.rolling_path
    q["rolling_over_trend"] = round(q["rolling_w5_ms"] / q["trend_ms"], 3)
    q["rolling_over_mean"] = round(q["rolling_w5_ms"] / q["mean_ms"], 3)
    q["result_shape"] = list(last["rolling_w5"].shape)
    got, parts = last["rolling_w5"], last["rolling_w5_components"]
    res["result"] = {"masked_outputs": int(np.ma.getmaskarray(got).sum()),
                     "valid_windows_mean": round(float(parts["n_windows"].mean()), 2),
                     "sum_max": float(got.max()), "position_max": int(parts["position"].max())}
    # a spot check against NumPy: two columns, windows summed oldest first
    col = data.view(torch.float32)
    spots = {}
    for j, k in ((5, 7), (700, 300)):
        pieces = []
        cj, ck = j // chunks[1], k // chunks[2]
        for l in range(grid[0]):
            o = int(offsets[(l * grid[1] + cj) * grid[2] + ck]) // 4
            pieces.append(col[o:o + cb // 4].view(*chunks)[:, j % chunks[1], k % chunks[2]])
        y = torch.cat(pieces).double().cpu().numpy()
        valid = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
        best = None
        for p in range(len(y) - 4):
            if valid[p:p + 5].all():
                s = y[p]
                for i in range(1, 5):
                    s = s + y[p + i]
                if best is None or s > best:
                    best = s
        spots[f"{j},{k}"] = {"got": None if np.ma.getmaskarray(got)[0, j, k] else float(got.data[0, j, k]),
                             "want": None if best is None else float(best)}
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
    rfin = DeviceBuffer(ctx, n_out * _lib.ROLL_NBYTES)
    rval = DeviceBuffer(ctx, n_out * 9)
    pfin = DeviceBuffer(ctx, n_out * _lib.PARTIAL_NBYTES)
    mval, mmask = DeviceBuffer(ctx, n_out * 8), DeviceBuffer(ctx, n_out)
    ctx.synchronize(st)

    def roll_chain(w):
        def chain():
            assert engine.roll_cols(ctx, plan.batch, plan.mask_up.struct, 0, w, "max", g, rfin.ptr, st)
            engine.roll_finalize(ctx, rfin.ptr, n_out, "sum", rval.ptr, rval.ptr + 8 * n_out, st)
            ctx.synchronize(st)
        return chain

    def roll_kernel():
        assert engine.roll_cols(ctx, plan.batch, plan.mask_up.struct, 0, 5, "max", g, rfin.ptr, st)
        ctx.synchronize(st)

    def spell_chain():
        assert engine.spell_cols(ctx, plan.batch, plan.mask_up.struct, 0, "lt", thr, 1, g, sfin.ptr, st)
        engine.spell_finalize(ctx, sfin.ptr, n_out, "longest", sval.ptr, sval.ptr + 4 * n_out, st)
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
    chains = {"mean": mean_chain, "trend": trend_chain, "spell": spell_chain}
    chains.update({f"rolling_w{w}": roll_chain(w) for w in WINDOWS})
    chains["rolling_w5_cols_only"] = roll_kernel
    for name, (med, lo) in timed_alternating(chains, a.reps, sync).items():
        d[name + "_ms"], d[name + "_ms_min"] = med, lo
    d["rolling_over_trend"] = round(d["rolling_w5_ms"] / d["trend_ms"], 3)
    d["rolling_over_spell"] = round(d["rolling_w5_ms"] / d["spell_ms"], 3)
    d["rolling_over_mean"] = round(d["rolling_w5_ms"] / d["mean_ms"], 3)
    for name in ("rolling_w5", "rolling_w8", "trend", "spell", "mean"):
        d["GBps_" + name] = round(n * cb / d[name + "_ms"] / 1e6, 1)
    release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
