"""Cost of k_start_feedback on one MI355X (not gated; DESIGN.md section 6 "Feedback hand-over"):

  device  256 windows, one launch of qtos_start_feedback_device between HIP events on the stream: median of 100 launches behind
          a warm-up launch, with the smallest and the largest
  host    the route it replaces: start, row and every window's measured row are read back, feedback.start_feedback runs in
          float64 numpy window by window, the corrected start vectors and goals are uploaded: wall clock around the three steps
          with the device idle before and after, median of 5

The windows are the golden walk handed over at rows spread over the plan, each measured 1 cm off its plan in a ring of 3000 rows.
Written to the JSON file named on the command line (profiles/feedback_cost.json is such a file)."""
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
    from qtos_amd import capi, feedback
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, cap = 256, 3000
    cfg = PlannerConfig.reference_compat()
    P = Planner(cfg, max_batch=B)
    dev = torch.device("cuda", 0)
    x = np.load(os.path.join(ROOT, "tests", "golden", "gv1.npz"))["x"]
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    nodes = torch.as_tensor(np.repeat(x[None], B, axis=0), **f64).contiguous()
    t0 = torch.zeros(B, **f64)
    stream = torch.cuda.current_stream(dev)
    sp_ = C.c_void_p(stream.cuda_stream)

    def chk(rc):
        assert rc == 0, P.lib.qtos_last_error(P.h)

    # the measured ring: the planned pose and the commanded angles of rows 0 .. cap - 1, 1 cm off in x
    joint, jst = torch.empty((B, cap, 37), **f64), torch.empty((B, cap), **i32)
    rows = torch.empty((B, cap, 37), **f64)
    jp = capi.joint_params(n_rows=cap)
    chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(jp), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None, joint.data_ptr(),
                                     jst.data_ptr(), sp_))
    chk(P.lib.qtos_sample_csv_device(P.h, B, nodes.data_ptr(), t0.data_ptr(), C.c_double(1000.0), cap, rows.data_ptr(), sp_))
    meas = torch.cat([rows[:, :, 1:7], joint[:, :, 1:13]], 2).contiguous()
    meas[:, :, 0] += 0.01
    row_np = (600 + 9 * np.arange(B)).astype(np.int32)                 # hand-over rows 600 .. 2895
    row = torch.as_tensor(row_np, **i32)
    start0 = rows[torch.arange(B, device=dev), row.long(), 1:25].contiguous()
    del joint, rows
    cursor = torch.zeros(B, dtype=torch.int64, device=dev)
    goal_step = torch.as_tensor(np.tile([0.3, 0.0, 0.0], (B, 1)), **f64)
    start, goal = start0.clone(), torch.zeros((B, 3), **f64)
    err, status = torch.zeros((B, 18), **f64), torch.zeros(B, **i32)
    p = capi.feedback_params(cfg, capacity=cap)
    res = dict(device=torch.cuda.get_device_name(0), windows=B)

    def launch():
        chk(P.lib.qtos_start_feedback_device(P.h, B, C.byref(p), nodes.data_ptr(), t0.data_ptr(), row.data_ptr(), cursor.data_ptr(),
                                             meas.data_ptr(), None, start.data_ptr(), goal_step.data_ptr(), goal.data_ptr(), err.data_ptr(),
                                             status.data_ptr(), sp_))
    launch()
    torch.cuda.synchronize()
    res["corrected_windows"] = int((status & 1).sum().item())
    ms = []
    for _ in range(100):
        start.copy_(start0)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        launch()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    res["device_launch_256"] = stats(ms)
    # the host route
    L, fp = sp.layout(cfg), feedback.FeedbackParams(capacity=cap)
    at = torch.as_tensor(row_np - 1, device=dev).long()
    ms, parts = [], []
    for _ in range(5):
        start.copy_(start0)
        torch.cuda.synchronize()
        a = time.perf_counter()
        s_h, r_h = start.cpu().numpy(), row.cpu().numpy()
        m_h = meas[torch.arange(B, device=dev), at].cpu().numpy()          # every window's measured row
        b = time.perf_counter()
        out, gl = np.empty((B, 24)), np.empty((B, 3))
        for w in range(B):
            ring = {int(r_h[w]) - 1: m_h[w]}
            o, g, _, _ = feedback.start_feedback(L, x, 0.0, int(r_h[w]), _OneRow(ring, cap), fp, s_h[w], None, 0, [0.3, 0.0, 0.0], 0, np.float64)
            out[w], gl[w, 0:2] = o, g
        c = time.perf_counter()
        start.copy_(torch.from_numpy(out))
        goal[:, 0:2].copy_(torch.from_numpy(gl[:, 0:2]))
        torch.cuda.synchronize()
        d = time.perf_counter()
        ms.append(1e3 * (d - a))
        parts.append((1e3 * (b - a), 1e3 * (c - b), 1e3 * (d - c)))
    res["host_route_256"] = stats(ms)
    mid = sorted(range(5), key=lambda i: ms[i])[2]
    res["host_route_parts_ms"] = dict(zip(("download", "numpy", "upload"), parts[mid]))
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


class _OneRow:
    """A measured ring of which one row was read back: indexed as the ring would be."""

    def __init__(self, rows, cap):
        self.rows, self.cap = rows, cap

    def __getitem__(self, i):
        return self.rows[int(i)]


if __name__ == "__main__":
    main()
