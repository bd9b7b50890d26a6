"""Active.grouped("mean", 0, labels, axis=(0,)) on the resident C3 variable
(1024^3 f32 in 64^3 chunks, _FillValue + valid_min / valid_max) for three label
vectors: i % 12 (a monthly climatology), blocks of 31 rows, and a DJF vector
that puts three quarters of the rows in no group.  Yardsticks measured in the
same run: mean(axis=(0,)), trend(0, coord, axis=(0,)) and the way to the same
numbers without grouped: the 12 queries var(axis=(0,))[rows of month g, :, :]
with components.

Device chains (launch to stream synchronise, on prepared plans): grouped =
pyas_group_cols; mean = pyas_reduce_axes_grid + pyas_format_partials; trend =
pyas_trend_cols + pyas_trend_finalize.  Whole queries: what the caller waits
for, records back on the host included.  Median of --reps after 3 warm-up
runs, in one process.

--stat names the grouped statistics to time, comma-separated (default: mean,
the output above unchanged).  Every other one ("max", "sum", "min") is timed
in the same process and run, after the yardsticks: its whole queries
(grouped_<stat>_<labels>) and its device chains, pyas_group_cols_partial alone
(..._kernel_ms: the same bytes read and 32-byte records written as the mean's
chain) and with the pyas_format_partials a query runs behind it (..._ms).

    python tools/bench_grouped.py [--reps 20] [--out profiles/grouped/bench_grouped.json]
    python tools/bench_grouped.py --stat mean,max,sum --out profiles/grouped_extremes/bench_grouped.json
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
    ap.add_argument("--out", default=os.path.join("profiles", "grouped", "bench_grouped.json"))
    ap.add_argument("--stat", default="mean",
                    help="grouped statistics to time, comma-separated; mean is always timed (default: mean)")
    ap.add_argument("--chains-only", action="store_true",
                    help="the device chains alone (for a counter run): no whole query, nothing written")
    a = ap.parse_args()
    a.extra = [s for s in dict.fromkeys(a.stat.split(",")) if s != "mean"]
    if any(s not in ("min", "max", "sum") for s in a.extra):
        ap.error("--stat takes mean, min, max and sum")
    import torch
    from pyactivestorage_amd.active import Active, attach_resident, release_resident
    from pyactivestorage_amd.synthetic import chunk_major_device
    from pyactivestorage_amd.variable import ChunkedVariable
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
    nt = shape[0]
    month = np.arange(nt) % 12
    vectors = {"mod12": (month, 12),
               "blocks31": (np.arange(nt) // 31, -(-nt // 31)),
               # December, January, February as one group; the other nine months in none
               "djf": (np.where(np.isin(month, (11, 0, 1)), 0, -1), 1)}
    days = np.array([31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31], dtype=np.float64)
    coord = 6e4 + np.concatenate([[0.0], np.cumsum(np.resize(days, nt - 1))])
    res = {"workload": f"resident C3 variable {tuple(shape)} {dt.str} in {tuple(chunks)} chunks, masked; "
                       "grouped('mean', 0, labels, axis=(0,))",
           "reps": a.reps, "queries": {}}
    act = Active(var, resident=True)
    comp = Active(var, resident=True)
    comp.components = True
    last = {}
    q = res["queries"]
    lists = [np.nonzero(month == g)[0].tolist() for g in range(12)]

    def twelve():
        return [comp.var(axis=(0,))[rows, :, :] for rows in lists]

    cases = [("mean", lambda: act.mean(axis=(0,))[...]),
             ("trend", lambda: act.trend(0, coord=coord, axis=(0,))[...]),
             ("twelve_listed_var_components", twelve)]
    for name, (lab, n_g) in vectors.items():
        cases.append(("grouped_" + name,
                      lambda lab=lab, n_g=n_g: act.grouped("mean", 0, lab, axis=(0,), n_groups=n_g)[...]))
    for stat in a.extra:
        for name, (lab, n_g) in vectors.items():
            cases.append((f"grouped_{stat}_{name}", lambda stat=stat, lab=lab, n_g=n_g:
                          act.grouped(stat, 0, lab, axis=(0,), n_groups=n_g)[...]))
    for name, fn in ([] if a.chains_only else cases):
        def run(name=name, fn=fn):
            last[name] = fn()
        q[name + "_ms"], q[name + "_ms_min"] = timed(run, a.reps, sync)
        print(json.dumps({name: q[name + "_ms"]}), flush=True)
    if not a.chains_only:
        spot_check(res, q, last, act, data, offsets, grid, cb, chunks, month, torch)
        for stat in a.extra:
            spot_check_stat(res, q, last, stat, data, offsets, grid, cb, chunks, month, torch)
    del last
    device_chains(res, a, vectors, data, offsets, grid, cb, chunks, shape, dt, attrs, coord, sync)
    release_resident(var)
    if a.chains_only:
        print(json.dumps(res["device_chain"]))
        return
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def spot_check(res, q, last, act, data, offsets, grid, cb, chunks, month, torch):
    """The grouped means against the 12 listed queries' means, and column (5, 7) against NumPy."""
    q["grouped_path"] = act.grouped_path
    q["twelve_over_grouped_mod12"] = round(q["twelve_listed_var_components_ms"] / q["grouped_mod12_ms"], 3)
    q["result_shape_mod12"] = list(last["grouped_mod12"].shape)
    want = np.ma.concatenate([c["mean"] for c in last["twelve_listed_var_components"]], axis=0)
    got = last["grouped_mod12"]
    err = np.abs(np.ma.getdata(got) - np.ma.getdata(want))[~np.ma.getmaskarray(want)]
    res["spot_check"] = {"masks_equal": bool(np.array_equal(np.ma.getmaskarray(got), np.ma.getmaskarray(want))),
                         "max_abs_diff_against_listed_queries": float(err.max())}
    col = data.view(torch.float32)
    ys = []
    for l in range(grid[0]):   # the chunks of column (5 // 64, 7 // 64) = (0, 0), layer l: chunk l * 256
        o = int(offsets[l * grid[1] * grid[2]]) // 4
        ys.append(col[o:o + cb // 4].view(*chunks)[:, 5, 7])
    y = torch.cat(ys).double().cpu().numpy()
    ok = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
    ref = np.array([y[ok & (month == g)].mean() for g in range(12)])
    res["spot_check"]["column_5_7_max_abs_err"] = float(np.abs(np.ma.getdata(got)[:, 5, 7] - ref).max())


def spot_check_stat(res, q, last, stat, data, offsets, grid, cb, chunks, month, torch):
    """min / max / sum of column (5, 7) against NumPy, and the whole query against the mean's."""
    q[f"grouped_{stat}_mod12_over_grouped_mod12"] = round(q[f"grouped_{stat}_mod12_ms"] / q["grouped_mod12_ms"], 3)
    got = last[f"grouped_{stat}_mod12"]
    col = data.view(torch.float32)
    ys = []
    for l in range(grid[0]):
        o = int(offsets[l * grid[1] * grid[2]]) // 4
        ys.append(col[o:o + cb // 4].view(*chunks)[:, 5, 7])
    y = torch.cat(ys).cpu().numpy()
    ok = (y != bench.FILL) & (y >= bench.VMIN) & (y <= bench.VMAX)
    fn = {"min": np.min, "max": np.max, "sum": lambda v: np.sum(v.astype(np.float64))}[stat]
    ref = np.array([fn(y[ok & (month == g)]) for g in range(12)])
    res["spot_check"][f"{stat}_dtype"] = str(got.dtype)
    res["spot_check"][f"{stat}_column_5_7_max_abs_err"] = float(np.abs(np.ma.getdata(got)[:, 5, 7].astype(np.float64)
                                                                        - ref).max())


def device_chains(res, a, vectors, data, offsets, grid, cb, chunks, shape, dt, attrs, coord, sync):
    """The device chains on prepared plans."""
    from pyactivestorage_amd import _lib, engine, grouped
    from pyactivestorage_amd.batch import ReductionPlan
    from pyactivestorage_amd.device import DeviceBuffer, get_context
    from pyactivestorage_amd.indexing import OrthogonalIndexer
    from pyactivestorage_amd.variable import get_missing_attributes
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
    tfin = DeviceBuffer(ctx, n_out * _lib.COMOMENTS_NBYTES)
    vbuf = DeviceBuffer(ctx, n_out * 9)
    pfin = DeviceBuffer(ctx, n_out * _lib.PARTIAL_NBYTES)
    mval, mmask = DeviceBuffer(ctx, n_out * 8), DeviceBuffer(ctx, n_out)
    dims0 = [list(OrthogonalIndexer((Ellipsis,), shape, chunks).dim_indexers[0])]
    chains = {}
    keep = []
    for name, (lab, n_g) in vectors.items():
        rows = grouped.row_list(dims0, chunks, np.asarray(lab, dtype=np.int64), 0, n_g)
        blob = np.concatenate([rows.layer, rows.offset, rows.label, np.zeros(1, dtype=np.int32)])
        rbuf = DeviceBuffer(ctx, blob.nbytes)
        ctx.h2d(rbuf.ptr, blob, st)
        fin = DeviceBuffer(ctx, n_g * n_out * _lib.MOMENTS_NBYTES)
        keep += [blob, rbuf, fin]

        def chain(rows=rows, rbuf=rbuf, fin=fin, n_g=n_g):
            assert engine.group_cols(ctx, plan.batch, plan.mask_up.struct, rbuf.ptr, rbuf.ptr + 4 * rows.n_rows,
                                     rbuf.ptr + 8 * rows.n_rows, rows.n_rows, n_g, g, fin.ptr, st)
            ctx.synchronize(st)
        chains["grouped_" + name] = (chain, rows.n_rows, n_g)
        for stat in a.extra:
            vdt = engine.format_dtype(dt, stat)
            val = DeviceBuffer(ctx, n_g * n_out * (vdt.itemsize + 1))
            keep.append(val)

            def kernel(rows=rows, rbuf=rbuf, fin=fin, n_g=n_g, sync_after=True):
                assert engine.group_cols(ctx, plan.batch, plan.mask_up.struct, rbuf.ptr, rbuf.ptr + 4 * rows.n_rows,
                                         rbuf.ptr + 8 * rows.n_rows, rows.n_rows, n_g, g, fin.ptr, st, partial=True)
                if sync_after:
                    ctx.synchronize(st)

            def formatted(kernel=kernel, fin=fin, n_g=n_g, val=val, vdt=vdt, stat=stat):
                kernel(sync_after=False)
                engine.format_partials(ctx, dt, fin.ptr, n_g * n_out, stat, val.ptr,
                                       val.ptr + n_g * n_out * vdt.itemsize, None, st)
                ctx.synchronize(st)
            chains[f"grouped_{stat}_{name}_kernel"] = (kernel, rows.n_rows, n_g)
            chains[f"grouped_{stat}_{name}"] = (formatted, rows.n_rows, n_g)
    ctx.synchronize(st)

    def trend_chain():
        assert engine.trend_cols(ctx, plan.batch, plan.mask_up.struct, cbuf.ptr, cbuf.ptr + cpool.nbytes, 0, g,
                                 tfin.ptr, st)
        engine.trend_finalize(ctx, tfin.ptr, n_out, _lib.TREND_SLOPE, vbuf.ptr, vbuf.ptr + 8 * n_out, st)
        ctx.synchronize(st)

    def mean_chain():
        engine.reduce_axes_grid(ctx, plan.batch, plan.mask_up.struct, g, pfin.ptr, True, st)
        engine.format_partials(ctx, dt, pfin.ptr, n_out, "mean", mval.ptr, mmask.ptr, None, st)
        ctx.synchronize(st)

    d = res["device_chain"] = {}
    for name, fn in (("mean", mean_chain), ("trend", trend_chain)):
        d[name + "_ms"], d[name + "_ms_min"] = timed(fn, a.reps, sync)
    for name, (fn, n_rows, n_g) in chains.items():
        d[name + "_ms"], d[name + "_ms_min"] = timed(fn, a.reps, sync)
        read = n_rows * n_out * dt.itemsize
        d[name + "_rows"], d[name + "_groups"] = n_rows, n_g
        d["GBps_" + name] = round((read + n_g * n_out * _lib.MOMENTS_NBYTES) / d[name + "_ms"] / 1e6, 1)
    d["grouped_mod12_over_mean"] = round(d["grouped_mod12_ms"] / d["mean_ms"], 3)
    d["grouped_mod12_over_trend"] = round(d["grouped_mod12_ms"] / d["trend_ms"], 3)
    d["djf_over_mod12"] = round(d["grouped_djf_ms"] / d["grouped_mod12_ms"], 3)
    d["GBps_mean"] = round(n * cb / d["mean_ms"] / 1e6, 1)
    for stat in a.extra:
        for name in vectors:
            for tail in ("", "_kernel"):
                d[f"grouped_{stat}_{name}{tail}_over_grouped_{name}"] = round(
                    d[f"grouped_{stat}_{name}{tail}_ms"] / d[f"grouped_{name}_ms"], 3)
        d[f"{stat}_djf_over_mod12"] = round(d[f"grouped_{stat}_djf_kernel_ms"] / d[f"grouped_{stat}_mod12_kernel_ms"], 3)
    del keep


if __name__ == "__main__":
    main()
