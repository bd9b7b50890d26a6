"""Active.mean(weights=...) against Active.mean on resident C3 (1024^3 f32 in
64^3 chunks, _FillValue + valid_min/valid_max, chunks attached in HBM), with
weights on dimension 1 only (cos-latitude) and on all three dimensions: whole
queries over all axes, (0,) and (2,), the unweighted mean of the same queries
in the same process, and for the full reduction the device chains alone
(launch to stream synchronise: pyas_wsum_axes + the record folds against
pyas_reduce_chunks).  Median of --reps after warm-up; writes a JSON.

    python tools/bench_weighted.py [--reps 20] [--out profiles/weighted/bench_weighted.json]
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
    ap.add_argument("--out", default=os.path.join("profiles", "weighted", "bench_weighted.json"))
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
    data, offsets, _ = chunk_major_device(torch, shape, chunks, dt, dev, fill=bench.FILL, fill_frac=0.01, seed=0)
    torch.cuda.synchronize()
    grid = [s // c for s, c in zip(shape, chunks)]
    cb = int(np.prod(chunks)) * dt.itemsize
    index = {co: (int(offsets[k]), cb) for k, co in enumerate(np.ndindex(*grid))}
    attrs = {"_FillValue": np.array([bench.FILL], dtype=dt), "valid_min": np.array([bench.VMIN], dtype=dt),
             "valid_max": np.array([bench.VMAX], dtype=dt)}
    var = ChunkedVariable(name="c3", shape=shape, chunks=chunks, dtype=dt, chunk_index=index, attrs=attrs,
                          filename=None, filter_pipeline=None)
    attach_resident(var, data.data_ptr(), device=0, owner=data)
    sync = torch.cuda.synchronize
    rng = np.random.default_rng(1)
    coslat = np.cos(np.linspace(-np.pi / 2, np.pi / 2, shape[1] + 2))[1:-1]
    wsets = {"dim1": {1: coslat},
             "dims012": {0: rng.uniform(0.5, 1.5, shape[0]), 1: coslat, 2: rng.uniform(0.5, 1.5, shape[2])}}
    res = {"workload": f"resident C3 {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked", "reps": a.reps,
           "queries": {}}
    act = Active(var, resident=True)
    last = {}
    for axis in (None, (0,), (2,)):
        row = {}

        def q_mean(axis=axis):
            last["mean"] = act.mean(axis=axis)[...]
        row["mean_ms"], row["mean_ms_min"] = timed(q_mean, a.reps, sync)
        for name, w in wsets.items():
            def q(axis=axis, w=w, name=name):
                last[name] = act.mean(axis=axis, weights=w)[...]
            row[name + "_ms"], row[name + "_ms_min"] = timed(q, a.reps, sync)
            row[name + "_over_mean"] = round(row[name + "_ms"] / row["mean_ms"], 3)
        row["result_shape"] = list(last["dim1"].shape)
        res["queries"][str(axis)] = row
        print(json.dumps({str(axis): row}), flush=True)
        if axis is None:   # against torch in float64 on the device (the chunk-major buffer, chunk by chunk)
            v = data.view(torch.float32).reshape(*grid, *chunks)
            ok = (v != bench.FILL) & (v >= bench.VMIN) & (v <= bench.VMAX)
            wl = torch.from_numpy(coslat.reshape(grid[1], chunks[1])).to(dev)
            W = wl.reshape(1, grid[1], 1, 1, chunks[1], 1).expand(v.shape)
            num = float(torch.where(ok, W * v.double(), torch.zeros((), dtype=torch.float64, device=dev)).sum())
            den = float(torch.where(ok, W, torch.zeros((), dtype=torch.float64, device=dev)).sum())
            res["full_wmean_dim1"] = float(last["dim1"].reshape(-1)[0])
            res["full_wmean_dim1_rel_err_vs_torch_f64"] = abs(res["full_wmean_dim1"] - num / den) / abs(num / den)
            del ok, W
    # the device chains of the full reduction on one prepared plan
    ctx = get_context(0)
    st = ctx.thread_stream()
    n = int(np.prod(grid))
    plan = ReductionPlan(ctx, dt, chunks, data.data_ptr(), np.asarray(offsets, dtype=np.int64),
                         missing=get_missing_attributes(attrs), stream=st)
    nb = _lib.WSUM_NBYTES
    recs, lvl1, fin = DeviceBuffer(ctx, n * nb), DeviceBuffer(ctx, (n // 64 + 1) * nb), DeviceBuffer(ctx, nb)
    seg1 = np.minimum(np.arange(-(-n // 64) + 1, dtype=np.int64) * 64, n)
    seg2 = np.array([0, seg1.size - 1], dtype=np.int64)
    sbuf = DeviceBuffer(ctx, seg1.nbytes + seg2.nbytes)
    ctx.h2d(sbuf.ptr, np.concatenate([seg1, seg2]), st)
    all_axes = (1 << len(chunks)) - 1
    coords = np.array(list(np.ndindex(*grid)), dtype=np.int64)
    tables = {}
    for name, w in wsets.items():
        act.weights = w
        pool, origin = act._weight_tables(coords)
        act.weights = None
        wbuf = DeviceBuffer(ctx, pool.nbytes + origin.nbytes)
        ctx.h2d(wbuf.ptr, pool, st)
        ctx.h2d(wbuf.ptr + pool.nbytes, origin, st)
        tables[name] = (wbuf, pool.nbytes, pool, origin)
    ctx.synchronize(st)

    def mean_chain():
        plan.launch(st, chunk_partials=False)
        ctx.synchronize(st)

    def wsum_chain(name):
        wbuf, off = tables[name][:2]
        engine.wsum_axes(ctx, plan.batch, plan.mask_up.struct, wbuf.ptr, wbuf.ptr + off, all_axes, None, recs.ptr, st)
        engine.wsum_combine_segments(ctx, recs.ptr, None, sbuf.ptr, seg1.size - 1, lvl1.ptr, st)
        engine.wsum_combine_segments(ctx, lvl1.ptr, None, sbuf.ptr + seg1.nbytes, 1, fin.ptr, st)
        ctx.synchronize(st)

    dev_full = res["device_full"] = {}
    dev_full["mean_ms"], dev_full["mean_ms_min"] = timed(mean_chain, a.reps, sync)
    for name in wsets:
        dev_full[name + "_ms"], dev_full[name + "_ms_min"] = timed(lambda: wsum_chain(name), a.reps, sync)
        dev_full[name + "_over_mean"] = round(dev_full[name + "_ms"] / dev_full["mean_ms"], 3)
        dev_full["GBps_" + name] = round(n * cb / dev_full[name + "_ms"] / 1e6, 1)
    release_resident(var)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
