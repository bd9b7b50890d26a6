"""Active.var / Active.cov with weights= against the unweighted queries, on two
resident C3 variables (1024^3 f32 in 64^3 chunks each, _FillValue +
valid_min/valid_max, chunks attached in HBM), with weights on dimensions 1
(cos-latitude) and 2.  For the axis sets None, (1, 2) and (0,): the device
chains (the record driver of a prepared query plan, launch to stream
synchronise: pyas_moments_axes / pyas_comoments_axes / pyas_wcomoments_axes +
the record combines) of var() against var(weights=...) and of cov(other)
against cov(other, weights=...), and the whole queries.  The yardstick is the
ratio the weighted mean has over the plain mean, re-measured here
in the same run: the device chains of pyas_reduce_chunks and pyas_wsum_axes
over all axes.  Median of --reps after warm-up; writes a JSON.

    python tools/bench_wmoments.py [--reps 20] [--out profiles/wmoments/bench_wmoments.json]
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
    ap.add_argument("--out", default=os.path.join("profiles", "wmoments", "bench_wmoments.json"))
    a = ap.parse_args()
    import torch
    from pyactivestorage_amd import _lib, engine
    from pyactivestorage_amd.active import Active, attach_resident, release_resident
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer
    from pyactivestorage_amd.indexing import OrthogonalIndexer
    from pyactivestorage_amd.synthetic import chunk_major_device
    from pyactivestorage_amd.variable import ChunkedVariable, get_missing_attributes
    cfg = bench.CONFIGS["c3"]
    dt = np.dtype(cfg["dtype"])
    shape, chunks = cfg["shape"], cfg["chunks"]
    dev = torch.device("cuda", 0)
    grid = [s // c for s, c in zip(shape, chunks)]
    cb = int(np.prod(chunks)) * dt.itemsize
    n = int(np.prod(grid))
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
    rng = np.random.default_rng(1)
    coslat = np.cos(np.linspace(-np.pi / 2, np.pi / 2, shape[1] + 2))[1:-1]
    w = {1: coslat, 2: rng.uniform(0.5, 1.5, shape[2])}
    res = {"workload": f"two resident C3 variables {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       "weights on dims 1 (cos-latitude) and 2", "reps": a.reps, "queries": {}, "device": {}}
    ax, ay = Active(sides[0][2], resident=True), Active(sides[1][2], resident=True)
    axis_sets = (None, (1, 2), (0,))
    last = {}
    # whole queries
    for axis in axis_sets:
        row = {}
        for name, q in (("var", lambda: ax.var(axis=axis)[...]), ("wvar", lambda: ax.var(axis=axis, weights=w)[...]),
                        ("cov", lambda: ax.cov(ay, axis=axis)[...]),
                        ("wcov", lambda: ax.cov(ay, axis=axis, weights=w)[...])):
            def run(name=name, q=q):
                last[name] = q()
            row[name + "_ms"], row[name + "_ms_min"] = timed(run, a.reps, sync)
        row["wvar_over_var"] = round(row["wvar_ms"] / row["var_ms"], 3)
        row["wcov_over_cov"] = round(row["wcov_ms"] / row["cov_ms"], 3)
        row["result_shape"] = list(last["wcov"].shape)
        res["queries"][str(axis)] = row
        print(json.dumps({str(axis): row}), flush=True)
        if axis is None:   # against torch in float64 on the device (the chunk-major buffers, chunk by chunk)
            vx = sides[0][0].view(torch.float32).reshape(*grid, *chunks)
            ok = (vx != bench.FILL) & (vx >= bench.VMIN) & (vx <= bench.VMAX)
            w1 = torch.from_numpy(w[1].reshape(grid[1], chunks[1])).to(dev).reshape(1, grid[1], 1, 1, chunks[1], 1)
            w2 = torch.from_numpy(w[2].reshape(grid[2], chunks[2])).to(dev).reshape(1, 1, grid[2], 1, 1, chunks[2])
            zero = torch.zeros((), dtype=torch.float64, device=dev)
            W = torch.where(ok, (w1 * w2).expand(vx.shape), zero)
            sw = float(W.sum())
            mean = float((W * vx.double()).sum()) / sw
            want = float((W * (vx.double() - mean) ** 2).sum()) / sw
            res["full_wvar"] = float(last["wvar"].reshape(-1)[0])
            res["full_wvar_rel_err_vs_torch_f64"] = abs(res["full_wvar"] - want) / want
            del vx, ok, W
    # the device chains: the record driver over a prepared query plan
    miss = get_missing_attributes(attrs)
    for axis in axis_sets:
        axes = tuple(range(len(shape))) if axis is None else axis
        ax.missing, ay.missing = miss, miss
        ax._held.stores = []
        q = ax._query_plan(OrthogonalIndexer(Ellipsis, tuple(shape), tuple(chunks)), None, None, axes, pair=ay)
        ctx, st = q.ctx, q.st
        pool, origin = ax._weight_tables(q.coords, ax._check_weights(w))
        wbuf = DeviceBuffer(ctx, pool.nbytes + origin.nbytes)
        ctx.h2d(wbuf.ptr, pool, st)
        ctx.h2d(wbuf.ptr + pool.nbytes, origin, st)
        ctx.synchronize(st)
        bx, mx, by, my = q.plan.batch, q.plan.mask_up.struct, q.plan_y.batch, q.plan_y.mask_up.struct

        def chain(nb, launch, segs, grids):
            def fn():
                ax._reduce_records(q, axes, nb, launch, segs, grids)
                ctx.synchronize(st)
            return fn
        chains = {
            "var": chain(_lib.MOMENTS_NBYTES,
                         lambda off, out: engine.moments_axes(ctx, bx, mx, q.axes_mask, off, out, st),
                         engine.moments_combine_segments, engine.moments_combine_grid),
            "wvar": chain(_lib.WCOMOMENTS_NBYTES,
                          lambda off, out: engine.wcomoments_axes(ctx, bx, mx, None, None, wbuf.ptr,
                                                                  wbuf.ptr + pool.nbytes, q.axes_mask, off, out, st),
                          engine.wcomoments_combine_segments, engine.wcomoments_combine_grid),
            "cov": chain(_lib.COMOMENTS_NBYTES,
                         lambda off, out: engine.comoments_axes(ctx, bx, mx, by, my, q.axes_mask, off, out, st),
                         engine.comoments_combine_segments, engine.comoments_combine_grid),
            "wcov": chain(_lib.WCOMOMENTS_NBYTES,
                          lambda off, out: engine.wcomoments_axes(ctx, bx, mx, by, my, wbuf.ptr,
                                                                  wbuf.ptr + pool.nbytes, q.axes_mask, off, out, st),
                          engine.wcomoments_combine_segments, engine.wcomoments_combine_grid),
        }
        d = {}
        for name, fn in chains.items():
            d[name + "_ms"], d[name + "_ms_min"] = timed(fn, a.reps, sync)
        d["wvar_over_var"] = round(d["wvar_ms"] / d["var_ms"], 3)
        d["wcov_over_cov"] = round(d["wcov_ms"] / d["cov_ms"], 3)
        for name, k in (("var", 1), ("wvar", 1), ("cov", 2), ("wcov", 2)):
            d["GBps_" + name] = round(k * n * cb / d[name + "_ms"] / 1e6, 1)
        res["device"][str(axis)] = d
        print(json.dumps({"device " + str(axis): d}), flush=True)
        if axis is None:   # the yardstick of DESIGN 6.8 in the same run: plain mean against weighted mean
            plan = ReductionPlan(ctx, dt, chunks, sides[0][0].data_ptr(), np.asarray(sides[0][1], dtype=np.int64),
                                 missing=miss, stream=st)

            def mean_chain():
                plan.launch(st, chunk_partials=False)
                ctx.synchronize(st)
            wmean = chain(_lib.WSUM_NBYTES,
                          lambda off, out: engine.wsum_axes(ctx, plan.batch, plan.mask_up.struct, wbuf.ptr,
                                                            wbuf.ptr + pool.nbytes, q.axes_mask, off, out, st),
                          engine.wsum_combine_segments, engine.wsum_combine_grid)
            y = res["yardstick_mean"] = {}
            y["mean_ms"], y["mean_ms_min"] = timed(mean_chain, a.reps, sync)
            y["wmean_ms"], y["wmean_ms_min"] = timed(wmean, a.reps, sync)
            y["wmean_over_mean"] = round(y["wmean_ms"] / y["mean_ms"], 3)
            y["GBps_mean"] = round(n * cb / y["mean_ms"] / 1e6, 1)
            y["GBps_wmean"] = round(n * cb / y["wmean_ms"] / 1e6, 1)
            print(json.dumps({"yardstick_mean": y}), flush=True)
        for store in ax._held.stores:
            from pyactivestorage_amd.active import _unhold
            _unhold(store)
        ax._held.stores = []
    for _, _, var in sides:
        release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
