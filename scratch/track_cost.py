"""Cost of k_track on one MI355X, between HIP events (not gated; DESIGN.md section 6 "Track kernel"):

  table   256 windows x 5001 rows, table mode
  tick    256 windows x 1 row each at a row of its own
  ring    256 windows, 2500 rows each into rings of 9000 rows: what a replan of ShiftedWindows(trajectory=9000, track=...) queues in
          front of its stitch

each next to the host route it replaces: the download of the measured rows and tracking.track_rows in float64 (numpy, timed on
a few windows and scaled to 256).  Medians of 20 runs with the smallest and the largest run, written to the JSON file named on
the command line (profiles/track_cost.json is such a file)."""
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
    from qtos_amd import capi, tracking
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, n_all, runs = 256, 5001, 20
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

    # the measured state: the planned pose and the commanded angles of the plan, with a perturbation
    joint, jst = torch.empty((B, n_all, 37), **f64), torch.empty((B, n_all), dtype=torch.int32, device=dev)
    rows = torch.empty((B, n_all, 37), **f64)
    jp = capi.joint_params(n_rows=n_all)
    chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(jp), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None, joint.data_ptr(),
                                     jst.data_ptr(), sp_))
    chk(P.lib.qtos_sample_csv_device(P.h, B, nodes.data_ptr(), t0.data_ptr(), C.c_double(1000.0), n_all, rows.data_ptr(), sp_))
    meas = (torch.cat([rows[:, :, 1:7], joint[:, :, 1:13]], 2) + 1e-3 * torch.randn((B, n_all, 18), **f64)).contiguous()
    del joint, rows
    count, total = torch.zeros((B, 2), dtype=torch.int64, device=dev), torch.zeros((B, 2), **f64)
    res = dict(device=torch.cuda.get_device_name(0), windows=B)
    # table
    table, status = torch.empty((B, n_all, 26), **f64), torch.empty((B, n_all), dtype=torch.int32, device=dev)
    p = capi.track_params(n_rows=n_all)
    res["table_256x5001"] = timed(lambda: chk(P.lib.qtos_track_device(P.h, B, C.byref(p), nodes.data_ptr(), t0.data_ptr(), None, None, None,
                                                                       meas.data_ptr(), None, count.data_ptr(), total.data_ptr(),
                                                                       table.data_ptr(), status.data_ptr(), sp_)))
    one = capi.track_params(n_rows=n_all)
    res["table_1x5001"] = timed(lambda: chk(P.lib.qtos_track_device(P.h, 1, C.byref(one), nodes.data_ptr(), t0.data_ptr(), None, None, None,
                                                                     meas.data_ptr(), None, count.data_ptr(), total.data_ptr(),
                                                                     table.data_ptr(), status.data_ptr(), sp_)))
    # tick
    first = torch.as_tensor(np.arange(B, dtype=np.int32) * 19 % n_all, device=dev)
    tick_meas = meas[:, 0:1, :].contiguous()
    tick, tick_st = torch.empty((B, 1, 26), **f64), torch.empty((B, 1), dtype=torch.int32, device=dev)
    goal_x = torch.zeros(B, **f64)
    pt = capi.track_params(n_rows=1)
    res["tick_256"] = timed(lambda: chk(P.lib.qtos_track_device(P.h, B, C.byref(pt), nodes.data_ptr(), t0.data_ptr(), first.data_ptr(), None, None,
                                                                 tick_meas.data_ptr(), goal_x.data_ptr(), count.data_ptr(), total.data_ptr(),
                                                                 tick.data_ptr(), tick_st.data_ptr(), sp_)), n=100)
    # ring: 2500 rows per window in front of the stitch
    cap = 9000
    ring, ring_st = torch.zeros((B, cap, 26), **f64), torch.zeros((B, cap), dtype=torch.int32, device=dev)
    ring_meas = torch.zeros((B, cap, 18), **f64)
    ring_meas[:, :n_all] = meas
    cursor = torch.full((B,), 7000, dtype=torch.int64, device=dev)            # (the segment wraps)
    n_rows = torch.full((B,), 2500, dtype=torch.int32, device=dev)
    pr = capi.track_params(capacity=cap)
    res["ring_256x2500"] = timed(lambda: chk(P.lib.qtos_track_device(P.h, B, C.byref(pr), nodes.data_ptr(), t0.data_ptr(), None, n_rows.data_ptr(),
                                                                      cursor.data_ptr(), ring_meas.data_ptr(), None, count.data_ptr(),
                                                                      total.data_ptr(), ring.data_ptr(), ring_st.data_ptr(), sp_)))
    # host route: download of the measured rows, numpy in float64
    host = {}
    for name, src in (("256x5001", meas), ("256x2500", meas[:, :2500].contiguous()), ("256x1", tick_meas)):
        ms = []
        for _ in range(5):
            torch.cuda.synchronize()
            a = time.perf_counter()
            src.cpu()
            ms.append(1e3 * (time.perf_counter() - a))
        host[name] = stats(ms)
    res["host_download"] = host
    L, tp = sp.layout(cfg), tracking.TrackParams()
    m0 = meas[0].cpu().numpy()
    numpy_ms = {}
    for name, n, reps in (("5001", n_all, 4), ("2500", 2500, 4), ("1", 1, 20)):
        ms = []
        for _ in range(reps):
            a = time.perf_counter()
            tracking.track_rows(L, x, 0.0, 1000.0, 0, n, m0[:n], tp, dtype=np.float64)
            ms.append(1e3 * (time.perf_counter() - a))
        numpy_ms[name] = stats(ms)
    res["host_numpy_per_window"] = numpy_ms
    res["host_route_ms_scaled"] = {
        "table_256x5001": host["256x5001"]["median_ms"] + B * numpy_ms["5001"]["median_ms"],
        "ring_256x2500": host["256x2500"]["median_ms"] + B * numpy_ms["2500"]["median_ms"],
        "tick_256": host["256x1"]["median_ms"] + B * numpy_ms["1"]["median_ms"],
    }
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
