"""Cost of k_force_fit on one MI355X, between HIP events (not gated; DESIGN.md section 6 "Force-fit kernel"):

  table+summary   256 windows x 5001 rows, the table with the feed-forward columns (a joint table is given) and the summary
  table           the same rows without the summary (no reductions)
  summary         the summary alone (no table is written)

against the numpy route it replaces: qtos_sample_csv_device and qtos_joint_rows_device, download of both tables, force_fit.fit_rows
in float64 (numpy, timed per window and scaled to 256).  Median of 100 launches after a warm-up with the smallest and the largest
run, and the bytes the launch has to write over its median time (its floor is that write: 256 x 5001 x 32 doubles), written to the
JSON file named on the command line (profiles/force_fit_cost.json is such a file)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    v = sorted(v)
    return dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1], runs=len(v))


def main():
    import torch
    from oracle import splines as sp
    from qtos_amd import capi, force_fit as ff, plan_check as pc
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, n_all, runs = 256, 5001, 100
    cfg = PlannerConfig.reference_compat()
    P = Planner(cfg, max_batch=B)
    dev = torch.device("cuda", 0)
    x = np.load(os.path.join(ROOT, "tests", "golden", "gv1.npz"))["x"]
    f64 = dict(dtype=torch.float64, device=dev)
    nodes = torch.as_tensor(np.repeat(x[None], B, axis=0), **f64).contiguous()
    t0 = torch.zeros(B, **f64)
    stream = torch.cuda.current_stream(dev)
    sp_ = C.c_void_p(stream.cuda_stream)

    def timed(fn, n=runs):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return stats(ms)

    def chk(rc):
        assert rc == 0, P.lib.qtos_last_error(P.h)

    res = dict(device=torch.cuda.get_device_name(0), windows=B, rows=n_all)
    joint = torch.empty((B, n_all, 37), **f64)
    jstatus = torch.empty((B, n_all), dtype=torch.int32, device=dev)
    jp = capi.joint_params(n_rows=n_all)
    joint_call = lambda: chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(jp), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None,
                                                          joint.data_ptr(), jstatus.data_ptr(), sp_))
    joint_call()
    table = torch.empty((B, n_all, capi.FIT_COLS), **f64)
    status = torch.empty((B, n_all), dtype=torch.int32, device=dev)
    summary = torch.as_tensor(ff.empty_summary(B).view(np.float64).reshape(B, 4, 3).copy(), **f64)
    p = capi.fit_params(cfg, n_rows=n_all)
    call = lambda jt, tb, st, sm: chk(P.lib.qtos_force_fit_device(P.h, B, C.byref(p), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, jt,
                                                                  None, tb, st, sm, sp_))
    res["table_and_summary_256x5001"] = timed(lambda: call(joint.data_ptr(), table.data_ptr(), status.data_ptr(), summary.data_ptr()))
    res["table_256x5001"] = timed(lambda: call(joint.data_ptr(), table.data_ptr(), status.data_ptr(), None))
    res["table_without_joint_256x5001"] = timed(lambda: call(None, table.data_ptr(), status.data_ptr(), None))
    res["summary_256x5001"] = timed(lambda: call(None, None, None, summary.data_ptr()))
    written = B * n_all * (capi.FIT_COLS * 8 + 4)
    res["table_bytes_written"] = written
    res["table_write_GBps_at_median"] = written / (1e-3 * res["table_256x5001"]["median_ms"]) / 1e9
    res["joint_rows_256x5001"] = timed(joint_call, n=20)
    rows = torch.empty((B, n_all, 37), **f64)
    sample = lambda: chk(P.lib.qtos_sample_csv_device(P.h, B, nodes.data_ptr(), t0.data_ptr(), C.c_double(1000.0), n_all, rows.data_ptr(), sp_))
    res["sample_csv_256x5001"] = timed(sample, n=20)
    # the numpy route: sample and joint rows on the device, download, numpy in float64
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        a = time.perf_counter()
        sample()
        joint_call()
        rows.cpu()
        jt = joint.cpu()
        ms.append(1e3 * (time.perf_counter() - a))
    res["host_sample_joint_and_download_256x5001"] = stats(ms)
    L = sp.layout(cfg)
    j0 = jt[0].numpy()
    ms = []
    for _ in range(5):
        a = time.perf_counter()
        t, _ = ff.fit_rows(L, x, 0.0, 1000.0, 0, n_all, cfg, joint=j0, dtype=np.float64)
        ff.summarise(t, 0, pc.stance_rows(L, 1000.0, 0, n_all), capi.FIT_TOL, cfg)
        ms.append(1e3 * (time.perf_counter() - a))
    res["host_numpy_per_window_5001"] = stats(ms)
    res["host_route_256x5001_ms_scaled"] = res["host_sample_joint_and_download_256x5001"]["median_ms"] + B * res["host_numpy_per_window_5001"]["median_ms"]
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
