"""Cost of k_rollout on one MI355X, between HIP events (reported, not gated; DESIGN.md section 6 "Rollout kernel"):

  table   256 windows x 5001 rows, table mode, substeps 1 and 4, with the joint table and the 20-column rows
  tick    256 windows x 1 row each at a row of its own, from the carried state
  ring    256 windows, 2500 rows each into rings of 9000 rows: what a replan of ShiftedWindows(trajectory=9000, rollout=...) queues in
          front of its track call

There is no earlier device or host route to compare with: the reference's robot is PyBullet, which this project never had.  Next
to the launch times stands the time of the float64 numpy statement (rollout.rollout_rows) per window, which is what a user
without the kernel would run.  Medians of 50 runs with the smallest and the largest run, written to the JSON file named on the
command line (profiles/rollout_cost.json is such a file)."""
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
    from qtos_amd import capi, rollout
    from qtos_amd.capi import Planner
    from qtos_amd.config import INERTIA_PHYSICAL, PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, n_all, runs = 256, 5001, 50
    cfg = PlannerConfig.reference_compat()
    P = Planner(cfg, max_batch=B)
    dev = torch.device("cuda", 0)
    x = np.load(os.path.join(ROOT, "tests", "golden", "gv1.npz"))["x"]
    f64 = dict(dtype=torch.float64, device=dev)
    nodes = torch.as_tensor(np.repeat(x[None], B, axis=0), **f64).contiguous()
    t0 = torch.zeros(B, **f64)
    stream = torch.cuda.current_stream(dev)
    sp_ = C.c_void_p(stream.cuda_stream)
    body = dict(cfg=cfg, inertia_b=INERTIA_PHYSICAL, kp_lin=300.0, kd_lin=30.0, kp_ang=30.0, kd_ang=1.0, f_fb_max=12.0)

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

    joint, jst = torch.empty((B, n_all, 37), **f64), torch.empty((B, n_all), dtype=torch.int32, device=dev)
    jp = capi.joint_params(n_rows=n_all)
    chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(jp), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None, joint.data_ptr(),
                                     jst.data_ptr(), sp_))
    state, count, word = torch.zeros((B, 13), **f64), torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    meas, rows = torch.empty((B, n_all, 18), **f64), torch.empty((B, n_all, 20), **f64)
    status = torch.empty((B, n_all), dtype=torch.int32, device=dev)
    res = dict(device=torch.cuda.get_device_name(0), windows=B, structure="one lane runs both chains of a window (no split, no pipeline over tiles)")

    def launch(p, nb, first=None, n_rows=None, cursor=None, jt=joint, m=meas, r=rows, s=status):
        ptr = lambda t: None if t is None else t.data_ptr()
        chk(P.lib.qtos_rollout_device(P.h, nb, C.byref(p), nodes.data_ptr(), t0.data_ptr(), ptr(first), ptr(n_rows), ptr(cursor), ptr(jt), None,
                                      None, state.data_ptr(), count.data_ptr(), word.data_ptr(), m.data_ptr(), ptr(r), s.data_ptr(), sp_))
    for sub in (1, 4):
        p = capi.rollout_params(n_rows=n_all, init=True, substeps=sub, **body)
        res["table_256x5001_substeps%d" % sub] = timed(lambda: launch(p, B))
        res["table_1x5001_substeps%d" % sub] = timed(lambda: launch(p, 1))
        bare = capi.rollout_params(n_rows=n_all, init=True, substeps=sub, **body)
        res["table_256x5001_substeps%d_meas_only" % sub] = timed(lambda: launch(bare, B, jt=None, r=None))
    assert int(word.max().item()) == 0
    # tick
    first = torch.as_tensor(np.arange(B, dtype=np.int32) * 19 % n_all, device=dev)
    tick_m, tick_r, tick_s = torch.empty((B, 1, 18), **f64), torch.empty((B, 1, 20), **f64), torch.empty((B, 1), dtype=torch.int32, device=dev)
    pt = capi.rollout_params(n_rows=1, init=True, **body)
    res["tick_256"] = timed(lambda: launch(pt, B, first=first, jt=None, m=tick_m, r=tick_r, s=tick_s), n=100)
    # ring: 2500 rows per window in front of the track call
    cap = 9000
    ring_m, ring_r = torch.zeros((B, cap, 18), **f64), torch.zeros((B, cap, 20), **f64)
    ring_s, ring_j = torch.zeros((B, cap), dtype=torch.int32, device=dev), torch.zeros((B, cap, 37), **f64)
    cursor = torch.full((B,), 7000, dtype=torch.int64, device=dev)            # (the segment wraps)
    n_rows = torch.full((B,), 2500, dtype=torch.int32, device=dev)
    pr = capi.rollout_params(capacity=cap, init=True, **body)
    res["ring_256x2500"] = timed(lambda: launch(pr, B, n_rows=n_rows, cursor=cursor, jt=ring_j, m=ring_m, r=ring_r, s=ring_s))
    # the float64 numpy statement, per window
    L = sp.layout(cfg)
    numpy_ms = {}
    for sub in (1, 4):
        rp = rollout.RolloutParams(**dict(body, substeps=sub))
        ms = []
        for _ in range(3):
            a = time.perf_counter()
            rollout.rollout_rows(L, x, 0.0, 1000.0, 0, n_all, rp, dtype=np.float64)
            ms.append(1e3 * (time.perf_counter() - a))
        numpy_ms["5001_substeps%d" % sub] = stats(ms)
    res["numpy_float64_statement_per_window"] = numpy_ms
    res["note"] = "no earlier device or host route exists (the reference's robot is PyBullet); the numpy statement per window stands in for one"
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
