"""Active.histogram against Active.mean on resident C3 (1024^3 f32 in 64^3
chunks, _FillValue + valid_min/valid_max, chunks attached in HBM): whole
queries over all axes with 64 and 2,048 uniform bins over the valid range and
with 64 bins over (0,) and (2,), the unweighted mean of the same queries in the
same process, and for the full reduction the device chains alone (launch to
stream synchronise: pyas_hist_reset + pyas_hist_axes against
pyas_reduce_chunks), also on a constant field (one hot bin) and on values
spread evenly over the bins.  The 64-bin counts are checked against torch in
float64 on the device.  Median of --reps after warm-up (a quarter of them for
the partial-axis histograms, which take a quarter of a second each); writes a
JSON.

    python tools/bench_hist.py [--reps 20] [--out profiles/hist/bench_hist.json]
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
    ap.add_argument("--out", default=os.path.join("profiles", "hist", "bench_hist.json"))
    ap.add_argument("--skip-axes", action="store_true", help="leave out the partial-axis queries")
    a = ap.parse_args()
    import torch
    from pyactivestorage_amd import engine, histogram
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
    rng_valid = (float(bench.VMIN), float(bench.VMAX))
    res = {"workload": f"resident C3 {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       f"uniform bins over {rng_valid}", "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    last = {}
    for axis in (None,) if a.skip_axes else (None, (0,), (2,)):
        row = {}

        def q_mean(axis=axis):
            last["mean"] = act.mean(axis=axis)[...]
        row["mean_ms"], row["mean_ms_min"] = timed(q_mean, a.reps, sync)
        for n_bins in (64, 2048) if axis is None else (64,):
            name = f"hist{n_bins}"

            def q(axis=axis, n_bins=n_bins, name=name):
                last[name] = act.histogram(n_bins, rng_valid, axis=axis)[...]
            reps = a.reps if axis is None else max(3, a.reps // 4)   # partial axes: one global atomic per element
            row[name + "_ms"], row[name + "_ms_min"] = timed(q, reps, sync)
            row[name + "_over_mean"] = round(row[name + "_ms"] / row["mean_ms"], 3)
        row["result_shape"] = list(last["hist64"].shape)
        res["queries"][str(axis)] = row
        print(json.dumps({str(axis): row}), flush=True)
        if axis is None:   # against torch in float64 on the device
            e = histogram.edges(64, rng_valid)
            v = data.view(torch.float32)
            ok = (v != bench.FILL) & (v >= bench.VMIN) & (v <= bench.VMAX)
            x = v[ok].double()
            del ok
            et = torch.from_numpy(e).to(dev)
            inside = x[(x >= et[0]) & (x <= et[-1])]
            idx = torch.clamp(torch.bucketize(inside, et, right=True) - 1, max=63)
            want = torch.bincount(idx, minlength=64).cpu().numpy()
            got = last["hist64"].reshape(-1)
            res["full_hist64_total"] = int(got.sum())
            res["full_hist64_equals_torch_f64"] = bool(np.array_equal(got, want))
            res["full_hist64_max_bin_share"] = round(float(got.max()) / max(int(got.sum()), 1), 4)
            del x, inside, idx
            torch.cuda.empty_cache()
    release_resident(var)
    # the device chains of the full reduction on prepared plans
    ctx = get_context(0)
    st = ctx.thread_stream()
    n = int(np.prod(grid))
    all_axes = (1 << len(chunks)) - 1
    missing = get_missing_attributes(attrs)
    offs = np.asarray(offsets, dtype=np.int64)

    def chains(buf, label, bin_counts):
        plan = ReductionPlan(ctx, dt, chunks, buf.data_ptr(), offs, missing=missing, stream=st)
        out = {}

        def mean_chain():
            plan.launch(st, chunk_partials=False)
            ctx.synchronize(st)
        out["mean_ms"], out["mean_ms_min"] = timed(mean_chain, a.reps, sync)
        for n_bins in bin_counts:
            e = histogram.edges(n_bins, rng_valid)
            ebuf, tbuf = DeviceBuffer(ctx, e.nbytes), DeviceBuffer(ctx, (n_bins + 3) * 8)
            ctx.h2d(ebuf.ptr, e, st)
            uniform = (e[0], n_bins / (e[-1] - e[0]))

            def hist_chain():
                engine.hist_reset(ctx, tbuf.ptr, 1, n_bins, st)
                engine.hist_axes(ctx, plan.batch, plan.mask_up.struct, ebuf.ptr, n_bins, uniform, all_axes, None,
                                 None, tbuf.ptr, st)
                ctx.synchronize(st)
            name = f"hist{n_bins}"
            out[name + "_ms"], out[name + "_ms_min"] = timed(hist_chain, a.reps, sync)
            out[name + "_over_mean"] = round(out[name + "_ms"] / out["mean_ms"], 3)
            out["GBps_" + name] = round(n * cb / out[name + "_ms"] / 1e6, 1)
            tab = np.zeros(n_bins + 3, np.int64)
            ctx.d2h(tab, tbuf.ptr, st)
            ctx.synchronize(st)
            out[name + "_max_bin_share"] = round(float(tab[:n_bins].max()) / max(int(tab.sum()), 1), 4)
            out[name + "_unmasked"] = int(tab.sum())
        res["device_full_" + label] = out
        print(json.dumps({label: out}), flush=True)

    chains(data, "c3", (64, 2048))
    del data
    torch.cuda.empty_cache()
    n_el = int(np.prod(shape))
    const = torch.full((n_el,), 2.5e8, dtype=torch.float32, device=dev)   # one hot bin
    chains(const.view(torch.uint8), "constant", (64,))
    del const
    torch.cuda.empty_cache()
    even = torch.empty(n_el, dtype=torch.float32, device=dev)             # every bin alike, neighbours unrelated
    even.uniform_(rng_valid[0], rng_valid[1], generator=torch.Generator(device=dev).manual_seed(0))
    chains(even.view(torch.uint8), "even", (64,))
    del even
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
