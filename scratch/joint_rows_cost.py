"""Cost of k_joint_rows on one MI355X, between HIP events (not gated; DESIGN.md section 6 "Joint-rows kernel"):

  table   256 windows x 5001 rows, table mode
  tick    256 windows x 1 row each at a row of its own, with the measured state
  ring    256 windows, 2500 rows each into a ring of 9000 rows: what a replan of ShiftedWindows(trajectory=9000, joints=...)
          queues in front of its stitch

against the host route: qtos_sample_csv_device, download of the rows, joints.joint_rows in float64 (numpy, timed on 8 windows and
scaled to 256).  Medians with the smallest and the largest run, written to the JSON file named on the command line
(profiles/joint_rows_cost.json is such a file)."""
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
    from qtos_amd import capi, joints
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

    res = dict(device=torch.cuda.get_device_name(0), windows=B)
    # table
    table, status = torch.empty((B, n_all, 37), **f64), torch.empty((B, n_all), dtype=torch.int32, device=dev)
    p = capi.joint_params(n_rows=n_all)
    res["table_256x5001"] = timed(lambda: chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(p), nodes.data_ptr(), t0.data_ptr(), None, None, None,
                                                                            None, None, table.data_ptr(), status.data_ptr(), sp_)))
    rows = torch.empty((B, n_all, 37), **f64)
    res["sample_csv_256x5001"] = timed(lambda: chk(P.lib.qtos_sample_csv_device(P.h, B, nodes.data_ptr(), t0.data_ptr(), C.c_double(1000.0),
                                                                                 n_all, rows.data_ptr(), sp_)))
    # tick
    first = torch.as_tensor(np.arange(B, dtype=np.int32) * 19 % n_all, device=dev)
    q_mes, qd_mes = torch.zeros((B, 12), **f64), torch.zeros((B, 12), **f64)
    tick, tick_st = torch.empty((B, 1, 37), **f64), torch.empty((B, 1), dtype=torch.int32, device=dev)
    pt = capi.joint_params(n_rows=1)
    res["tick_256"] = timed(lambda: chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(pt), nodes.data_ptr(), t0.data_ptr(), first.data_ptr(), None,
                                                                     None, q_mes.data_ptr(), qd_mes.data_ptr(), tick.data_ptr(),
                                                                     tick_st.data_ptr(), sp_)), n=100)
    # ring: 2500 rows per window in front of the stitch, and the stitch itself
    cap = 9000
    ring, ring_st = torch.zeros((B, cap, 37), **f64), torch.zeros((B, cap), dtype=torch.int32, device=dev)
    csv_ring, cursor = torch.zeros((B, cap, 37), **f64), torch.zeros(B, dtype=torch.int64, device=dev)
    n_rows = torch.full((B,), 2500, dtype=torch.int32, device=dev)
    pr, s = capi.joint_params(capacity=cap), capi.stitch_params(cap, 0, 0, 1000.0, True)
    res["ring_joint_256x2500"] = timed(lambda: chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(pr), nodes.data_ptr(), t0.data_ptr(), None,
                                                                                 n_rows.data_ptr(), cursor.data_ptr(), None, None,
                                                                                 ring.data_ptr(), ring_st.data_ptr(), sp_)))
    res["ring_stitch_256x2500"] = timed(lambda: chk(P.lib.qtos_stitch_device(P.h, B, C.byref(s), nodes.data_ptr(), n_rows.data_ptr(),
                                                                              t0.data_ptr(), csv_ring.data_ptr(), cursor.data_ptr(), sp_)))
    # host route: sample on the device, download, numpy in float64
    ms = []
    for _ in range(5):
        torch.cuda.synchronize()
        a = time.perf_counter()
        chk(P.lib.qtos_sample_csv_device(P.h, B, nodes.data_ptr(), t0.data_ptr(), C.c_double(1000.0), n_all, rows.data_ptr(), sp_))
        rows.cpu()
        ms.append(1e3 * (time.perf_counter() - a))
    res["host_sample_and_download_256x5001"] = stats(ms)
    L, jp = sp.layout(cfg), joints.JointParams()
    ms = []
    for _ in range(8):
        a = time.perf_counter()
        joints.joint_rows(L, x, 0.0, 1000.0, 0, n_all, jp, dtype=np.float64)
        ms.append(1e3 * (time.perf_counter() - a))
    res["host_numpy_per_window_5001"] = stats(ms)
    res["host_route_256x5001_ms_scaled"] = res["host_sample_and_download_256x5001"]["median_ms"] + B * res["host_numpy_per_window_5001"]["median_ms"]
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
