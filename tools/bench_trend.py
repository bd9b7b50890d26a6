"""Active.trend(along=0, axis=(0,)) on the resident C3 variable (1024^3 f32 in
64^3 chunks, _FillValue + valid_min/valid_max, chunks attached in HBM) against
an irregular coordinate, with its two yardsticks measured in the same run:
mean(axis=(0,)), which reads the same bytes through the dense fold, and
cov(self, axis=(0,)), the only per-point co-moment query without trend.

Device chains (launch to stream synchronise, on prepared plans): trend =
pyas_trend_cols + pyas_trend_finalize; mean = pyas_reduce_axes_grid +
pyas_format_partials.  Whole queries: trend (the slope), trend with
components, mean and cov.  Reported: trend / mean for the device chain and
trend / cov for the whole query (which must come out below 1).  Median of
--reps after warm-up, one process; writes a JSON.

    python tools/bench_trend.py [--reps 20] [--out profiles/trend/bench_trend.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "trend", "bench_trend.json"))
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
    # irregular: cumulative month lengths from day 60,000
    days = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], dtype=np.float64)
    coord = 6e4 + np.concatenate([[0.0], np.cumsum(np.resize(days, shape[0] - 1))])
    res = {"workload": f"resident C3 variable {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       "trend(along=0, axis=(0,)) against cumulative month lengths",
           "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    comp = Active(var, resident=True)
    comp.components = True
    last = {}
    q = res["queries"]
    for name, fn in (("mean", lambda: act.mean(axis=(0,))[...]),
                     ("cov_self", lambda: act.cov(act, axis=(0,))[...]),
                     ("trend", lambda: act.trend(0, coord=coord, axis=(0,))[...]),
                     ("trend_components", lambda: comp.trend(0, coord=coord, axis=(0,))[...])):
        def run(name=name, fn=fn):
            last[name] = fn()
        q[name + "_ms"], q[name + "_ms_min"] = timed(run, a.reps, sync)
        print(json.dumps({name: q[name + "_ms"]}), flush=True)
    q["trend_path"] = act.trend_path
    q["trend_over_cov"] = round(q["trend_ms"] / q["cov_self_ms"], 3)
    q["trend_components_over_cov"] = round(q["trend_components_ms"] / q["cov_self_ms"], 3)
    q["trend_over_mean"] = round(q["trend_ms"] / q["mean_ms"], 3)
    q["result_shape"] = list(last["trend"].shape)
    # a spot check against torch in float64 on the device: column (0, 5, 7)
    col = data.view(torch.float32)
    ok_cols = []
    n0 = grid[0]
    for l in range(n0):   # the chunks of column (5 // 64, 7 // 64) = (0, 0), layer l: chunk l * 256
        o = int(offsets[l * grid[1] * grid[2]]) // 4
        ch = col[o:o + cb // 4].view(*chunks)
        ok_cols.append(ch[:, 5, 7])
    y = torch.cat(ok_cols).double().cpu().numpy()
    ok = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
    xs, ys = coord[ok], y[ok]
    want = float(((xs - xs.mean()) * (ys - ys.mean())).sum() / ((xs - xs.mean()) ** 2).sum())
    got = float(last["trend"][0, 5, 7])
    scale = float(np.sqrt(((ys - ys.mean()) ** 2).sum() / ((xs - xs.mean()) ** 2).sum()))
    res["spot_check"] = {"got": got, "want": want, "err_over_scale": abs(got - want) / scale if scale else 0.0}
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
    cpool = np.ascontiguousarray(coord)
    corigin = (np.array([co[0] for co in np.ndindex(*grid)], dtype=np.int64) * chunks[0]).astype(np.int32)
    cbuf = DeviceBuffer(ctx, cpool.nbytes + corigin.nbytes)
    ctx.h2d(cbuf.ptr, cpool, st)
    ctx.h2d(cbuf.ptr + cpool.nbytes, corigin, st)
    fin = DeviceBuffer(ctx, n_out * _lib.COMOMENTS_NBYTES)
    vbuf = DeviceBuffer(ctx, n_out * 9)
    pfin = DeviceBuffer(ctx, n_out * _lib.PARTIAL_NBYTES)
    mval, mmask = DeviceBuffer(ctx, n_out * 8), DeviceBuffer(ctx, n_out)
    ctx.synchronize(st)

    def trend_chain():
        assert engine.trend_cols(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, 0, g,
                                 fin.ptr, st)
        engine.trend_finalize(ctx, fin.ptr, n_out, _lib.TREND_SLOPE, vbuf.ptr, vbuf.ptr + 8 * n_out, st)
        ctx.synchronize(st)

    def trend_kernel():
        assert engine.trend_cols(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, 0, g,
                                 fin.ptr, st)
        ctx.synchronize(st)

    def mean_chain():
        engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, pfin.ptr, True, st)
        engine.format_partials(ctx, dt, pfin.ptr, n_out, "mean", mval.ptr, mmask.ptr, None, st)
        ctx.synchronize(st)

    d = res["device_chain"] = {}
    for name, fn in (("mean", mean_chain), ("trend", trend_chain), ("trend_cols_only", trend_kernel)):
        d[name + "_ms"], d[name + "_ms_min"] = timed(fn, a.reps, sync)
    d["trend_over_mean"] = round(d["trend_ms"] / d["mean_ms"], 3)
    d["GBps_trend"] = round(n * cb / d["trend_ms"] / 1e6, 1)
    d["GBps_mean"] = round(n * cb / d["mean_ms"] / 1e6, 1)
    release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
