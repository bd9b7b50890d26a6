"""Active.cov against the two Active.var passes over the same bytes, on two
resident C3 variables (1024^3 f32 in 64^3 chunks each, _FillValue +
valid_min/valid_max, chunks attached in HBM).  The yardstick: the device chain
of cov over all axes (launch to stream synchronise: pyas_comoments_axes + the
record folds) against the sum of the device chains of var(x) and var(y), each
run alone in the same process; target cov <= 1.10 x that sum.  Whole queries
over all axes, (0,) and (2,) are recorded without a target.  (Both variables
hold the synthetic ramp, under different fill plantings: their correlation is
1, which the timings do not depend on.)  Median of --reps after warm-up;
writes a JSON.

    python tools/bench_comoments.py [--reps 20] [--out profiles/comoments/bench_comoments.json]
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
    ap.add_argument("--out", default=os.path.join("profiles", "comoments", "bench_comoments.json"))
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
    sides = []
    for seed in (0, 1):
        data, offsets, _ = chunk_major_device(torch, shape, chunks, dt, dev, fill=bench.FILL, fill_frac=0.01, seed=seed)
        index = {co: (int(offsets[k]), cb) for k, co in enumerate(np.ndindex(*grid))}
        var = ChunkedVariable(name=f"c3_{seed}", shape=shape, chunks=chunks, dtype=dt, chunk_index=index, attrs=attrs,
                              filename=None, filter_pipeline=None)
        attach_resident(var, data.data_ptr(), device=0, owner=data)
        sides.append((data, offsets, var))
    torch.cuda.synchronize()
    sync = torch.cuda.synchronize
    res = {"workload": f"two resident C3 variables {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked",
           "reps": a.reps, "queries": {}}
    ax, ay = Active(sides[0][2], resident=True), Active(sides[1][2], resident=True)
    last = {}
    for axis in (None, (0,), (2,)):
        row = {}
        for name, q in (("var_x", lambda: ax.var(axis=axis)[...]), ("var_y", lambda: ay.var(axis=axis)[...]),
                        ("cov", lambda: ax.cov(ay, axis=axis)[...]), ("corr", lambda: ax.corr(ay, axis=axis)[...])):
            def run(name=name, q=q):
                last[name] = q()
            row[name + "_ms"], row[name + "_ms_min"] = timed(run, a.reps, sync)
        row["cov_over_two_vars"] = round(row["cov_ms"] / (row["var_x_ms"] + row["var_y_ms"]), 3)
        row["result_shape"] = list(last["cov"].shape)
        res["queries"][str(axis)] = row
        print(json.dumps({str(axis): row}), flush=True)
        if axis is None:   # against torch in float64 on the device
            vx, vy = sides[0][0].view(torch.float32), sides[1][0].view(torch.float32)
            ok = (vx != bench.FILL) & (vx >= bench.VMIN) & (vx <= bench.VMAX)
            ok &= (vy != bench.FILL) & (vy >= bench.VMIN) & (vy <= bench.VMAX)
            x, y = vx[ok].double(), vy[ok].double()
            dx, dy = x - x.mean(), y - y.mean()
            want = float((dx * dy).sum() / x.numel())
            scale = float(torch.sqrt((dx * dx).sum() * (dy * dy).sum()) / x.numel())
            res["full_cov"] = float(last["cov"].reshape(-1)[0])
            res["full_corr"] = float(last["corr"].reshape(-1)[0])
            res["full_cov_err_over_scale_vs_torch_f64"] = abs(res["full_cov"] - want) / scale
            del x, y, dx, dy, ok
    # the device chains of the full reduction on prepared plans
    ctx = get_context(0)
    st = ctx.thread_stream()
    n = int(np.prod(grid))
    plans = [ReductionPlan(ctx, dt, chunks, data.data_ptr(), np.asarray(offsets, dtype=np.int64),
                           missing=get_missing_attributes(attrs), stream=st) for data, offsets, _ in sides]
    seg1 = np.minimum(np.arange(-(-n // 64) + 1, dtype=np.int64) * 64, n)
    seg2 = np.array([0, seg1.size - 1], dtype=np.int64)
    sbuf = DeviceBuffer(ctx, seg1.nbytes + seg2.nbytes)
    ctx.h2d(sbuf.ptr, np.concatenate([seg1, seg2]), st)
    all_axes = (1 << len(chunks)) - 1
    nb = _lib.COMOMENTS_NBYTES     # (the larger record: the buffers serve both chains)
    recs, lvl1, fin = DeviceBuffer(ctx, n * nb), DeviceBuffer(ctx, (n // 64 + 1) * nb), DeviceBuffer(ctx, nb)

    def var_chain(plan):
        engine.moments_axes(ctx, plan.batch, plan.mask_up.struct, all_axes, None, recs.ptr, st)
        engine.moments_combine_segments(ctx, recs.ptr, None, sbuf.ptr, seg1.size - 1, lvl1.ptr, st)
        engine.moments_combine_segments(ctx, lvl1.ptr, None, sbuf.ptr + seg1.nbytes, 1, fin.ptr, st)
        ctx.synchronize(st)

    def cov_chain():
        engine.comoments_axes(ctx, plans[0].batch, plans[0].mask_up.struct, plans[1].batch, plans[1].mask_up.struct,
                              all_axes, None, recs.ptr, st)
        engine.comoments_combine_segments(ctx, recs.ptr, None, sbuf.ptr, seg1.size - 1, lvl1.ptr, st)
        engine.comoments_combine_segments(ctx, lvl1.ptr, None, sbuf.ptr + seg1.nbytes, 1, fin.ptr, st)
        ctx.synchronize(st)

    d = res["device_full"] = {}
    for name, fn in (("var_x", lambda: var_chain(plans[0])), ("var_y", lambda: var_chain(plans[1])),
                     ("cov", cov_chain)):
        d[name + "_ms"], d[name + "_ms_min"] = timed(fn, a.reps, sync)
    d["cov_over_two_vars"] = round(d["cov_ms"] / (d["var_x_ms"] + d["var_y_ms"]), 3)
    d["target"] = 1.10
    d["GBps_cov"] = round(2 * n * cb / d["cov_ms"] / 1e6, 1)
    d["GBps_var_x"] = round(n * cb / d["var_x_ms"] / 1e6, 1)
    for _, _, var in sides:
        release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
