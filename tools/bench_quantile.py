"""Active.median against Active.mean on resident C3 (1024^3 f32 in 64^3
chunks, _FillValue + valid_min/valid_max, chunks attached in HBM): the whole
median query over all axes at digit widths 8 and 11 and over (0,) and (2,) at
the default width, the unweighted mean of the same queries in the same
process, and for the full reduction the device chain of one order statistic
alone (launch to stream synchronise: every pass's pyas_hist_reset +
pyas_select_axes + pyas_select_step, against pyas_reduce_chunks) at both
widths.  The full median is checked against a float32 sort in torch on the
device.  Median of --reps after warm-up (3 for the partial-axis queries, which
count with one global atomic per element and pass); writes a JSON.

    python tools/bench_quantile.py [--reps 20] [--out profiles/quantile/bench_quantile.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def timed(fn, reps, sync, warm=3):
    for _ in range(warm):
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
    ap.add_argument("--out", default=os.path.join("profiles", "quantile", "bench_quantile.json"))
    ap.add_argument("--skip-axes", action="store_true", help="leave out the partial-axis queries")
    a = ap.parse_args()
    import torch
    from pyactivestorage_amd import engine, quantile
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
    default_bits = quantile.DIGIT_BITS
    res = {"workload": f"resident C3 {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; median",
           "reps": a.reps, "default_digit_bits": default_bits, "queries": {}}
    act = Active(var, resident=True)
    last = {}
    for axis in (None,) if a.skip_axes else (None, (0,), (2,)):
        row = {}

        def q_mean(axis=axis):
            last["mean"] = act.mean(axis=axis)[...]
        row["mean_ms"], row["mean_ms_min"] = timed(q_mean, a.reps, sync)
        for bits in (8, 11) if axis is None else (default_bits,):
            name = f"median_bits{bits}"
            quantile.DIGIT_BITS = bits

            def q(axis=axis, name=name):
                c = act.components
                act.components = True
                last[name] = act.median(axis=axis)[...]
                act.components = c
            reps, warm = (a.reps, 3) if axis is None else (3, 1)
            row[name + "_ms"], row[name + "_ms_min"] = timed(q, reps, sync, warm)
            row[name + "_over_mean"] = round(row[name + "_ms"] / row["mean_ms"], 3)
            row[name + "_count_passes"] = act._select_stats["passes"]
            row[name + "_chains"] = act._select_stats["chains"]
            row[name + "_digit_bits"] = act._select_stats["bits"]
        quantile.DIGIT_BITS = default_bits
        row["result_shape"] = list(last[name]["quantile"].shape)
        res["queries"][str(axis)] = row
        print(json.dumps({str(axis): row}), flush=True)
        if axis is None:   # against a float32 sort on the device
            v = data.view(torch.float32)
            ok = (v != bench.FILL) & (v >= bench.VMIN) & (v <= bench.VMAX)
            x = torch.sort(v[ok]).values
            del ok
            n = int(x.numel())
            h, lo, hi = quantile.ranks(n, 0.5, "linear")
            want = quantile.finalize(float(x[int(lo)]), float(x[int(hi)]), h, "linear")
            got8 = float(np.ma.getdata(last["median_bits8"]["quantile"]).reshape(-1)[0])
            got11 = float(np.ma.getdata(last["median_bits11"]["quantile"]).reshape(-1)[0])
            res["full_median"] = got8
            res["full_n"] = int(last["median_bits8"]["n"].reshape(-1)[0])
            res["full_median_equals_torch_sort"] = bool(got8 == float(want) and got11 == float(want) and res["full_n"] == n)
            del x
            torch.cuda.empty_cache()
    release_resident(var)
    # the device chain of one order statistic of the full reduction on a prepared plan
    ctx = get_context(0)
    st = ctx.thread_stream()
    n_chunks = int(np.prod(grid))
    all_axes = (1 << len(chunks)) - 1
    missing = get_missing_attributes(attrs)
    offs = np.asarray(offsets, dtype=np.int64)
    plan = ReductionPlan(ctx, dt, chunks, data.data_ptr(), offs, missing=missing, stream=st)
    out = {}

    def mean_chain():
        plan.launch(st, chunk_partials=False)
        ctx.synchronize(st)
    out["mean_ms"], out["mean_ms_min"] = timed(mean_chain, a.reps, sync)
    rank = np.array([(res.get("full_n", 2) - 1) // 2], dtype=np.int64)
    work = DeviceBuffer(ctx, 16)
    for bits in (8, 11):
        passes = quantile.digits(quantile.key_width(dt), bits)
        tbuf = DeviceBuffer(ctx, ((1 << bits) + 3) * 8)

        def select_chain(passes=passes, tbuf=tbuf):
            ctx.h2d(work.ptr, np.concatenate([rank, np.zeros(1, np.int64)]), st)   # the rank, then prefix 0
            for k, (shift, b) in enumerate(passes):
                engine.hist_reset(ctx, tbuf.ptr, 1, 1 << b, st)
                engine.select_axes(ctx, plan.batch, plan.mask_up.struct, work.ptr + 8 if k else None, shift, b,
                                   all_axes, None, None, tbuf.ptr, st)
                engine.select_step(ctx, tbuf.ptr, 1, b, work.ptr, work.ptr + 8, None, st)
            ctx.synchronize(st)
        name = f"select_bits{bits}"
        out[name + "_ms"], out[name + "_ms_min"] = timed(select_chain, a.reps, sync)
        out[name + "_passes"] = len(passes)
        out[name + "_over_mean"] = round(out[name + "_ms"] / out["mean_ms"], 3)
        out[name + "_per_pass_over_mean"] = round(out[name + "_ms"] / out["mean_ms"] / len(passes), 3)
        out[name + "_within_target"] = bool(out[name + "_ms"] <= len(passes) * 1.5 * out["mean_ms"])
        out["GBps_per_pass_" + name] = round(n_chunks * cb * len(passes) / out[name + "_ms"] / 1e6, 1)
        key = np.zeros(1, np.uint64)
        ctx.d2h(key, work.ptr + 8, st)
        ctx.synchronize(st)
        out[name + "_value"] = float(quantile.values(key, dt)[0])
    res["device_full_c3"] = out
    print(json.dumps({"device_full_c3": out}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
