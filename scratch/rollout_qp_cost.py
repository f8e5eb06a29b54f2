"""Cost of k_rollout_qp next to k_rollout_feet with QTOS_FEET_LIMIT on one MI355X, on the same inputs in the same run, between HIP
events (not gated; DESIGN.md section 6 "Rollout with the force QP"):

  table_256x5001_mu0.5_fmax30    256 windows x 5001 rows of the device's trot at 1 kHz, tables, joint table given, mu 0.5 / 30 N
  table_256x5001_mu0.5_fmax16    the same at mu 0.5 / 16 N (the cap below the trot's share of the weight: most ticks limited)
  tick_256x1                     the one-row tick (the 64-lane instantiation) at mu 0.5 / 16 N, from the plan's own state

with the gains of tests/rollout_cases.py on the physical inertia, damping 1e-2, substeps 1, dev_max 0.5 m and tilt_max 1 rad (a body
that falls is frozen, and a frozen row costs nothing: the share of frozen and of limited rows is written beside every time; the
carried word and count are zeroed in front of every launch, outside the events).
Median of the launches after a warm-up of 3, with the smallest and the largest run; per kernel the time per tick of one window's
chain (median / rows: the windows run side by side, one workgroup each).  Written to the JSON file named on the command line
(profiles/rollout_qp_cost.json is such a file)."""
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    v = sorted(v)
    return dict(median_ms=v[len(v) // 2], min_ms=v[0], max_ms=v[-1], runs=len(v))


def main():
    import torch
    import rollout_cases as rc
    from qtos_amd import capi, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import INERTIA_PHYSICAL, PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, n_all = 256, 5001
    cfg = PlannerConfig.reference_compat(gait="trot")
    P = Planner(cfg, max_batch=B)
    dev = torch.device("cuda", 0)
    start = workloads.rest_start(0.1)[None]
    x, status, _, _ = P.plan(start, np.array([[0.1 + 0.09 * cfg.duration, 0.0, 0.24]]))
    assert status[0] == 0
    f64 = dict(dtype=torch.float64, device=dev)
    nodes = torch.as_tensor(np.repeat(x, B, axis=0), **f64).contiguous()
    t0 = torch.zeros(B, **f64)
    stream = torch.cuda.current_stream(dev)
    sp_ = C.c_void_p(stream.cuda_stream)

    def timed(fn, runs, prep):
        for _ in range(3):
            prep()
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            prep()                                     # (outside the events: a fallen window's word is sticky, so every launch starts clean)
            a.record(stream)
            fn()
            b.record(stream)
            b.synchronize()
            ms.append(a.elapsed_time(b))
        return stats(ms)

    def chk(rc_):
        assert rc_ == 0, P.lib.qtos_last_error(P.h)

    res = dict(device=torch.cuda.get_device_name(0), windows=B, plan="the device's trot (PlannerConfig.reference_compat(gait='trot'))")
    body = dict(cfg=cfg, inertia_b=INERTIA_PHYSICAL, dev_max=0.5, tilt_max=1.0, **rc.GAINS)

    def case(name, rows, f_max, runs, first=0):
        joint = torch.zeros((B, rows, 37), **f64)
        jstatus = torch.zeros((B, rows), dtype=torch.int32, device=dev)
        chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(capi.joint_params(first_row=first, n_rows=rows)), nodes.data_ptr(), t0.data_ptr(), None, None,
                                         None, None, None, joint.data_ptr(), jstatus.data_ptr(), sp_))
        meas, table, ftable, qtable = (torch.zeros((B, rows, c), **f64) for c in (18, 20, 16, 8))
        status = torch.zeros((B, rows), dtype=torch.int32, device=dev)
        state, count, word = torch.zeros((B, 13), **f64), torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        kw = dict(hz=1000.0, substeps=1, first_row=first, n_rows=rows, init=True, mu=0.5, f_max=f_max, damping=1e-2, **body)
        clip, qp = capi.rollout_feet_params(limit=True, **kw), capi.rollout_qp_params(**kw)
        common = (nodes.data_ptr(), t0.data_ptr(), None, None, None, joint.data_ptr(), None, None, state.data_ptr(), count.data_ptr(), word.data_ptr(),
                  meas.data_ptr(), table.data_ptr(), ftable.data_ptr())
        run_clip = lambda: chk(P.lib.qtos_rollout_feet_device(P.h, B, C.byref(clip), *common, status.data_ptr(), sp_))
        run_qp = lambda: chk(P.lib.qtos_rollout_qp_device(P.h, B, C.byref(qp), *common, qtable.data_ptr(), status.data_ptr(), sp_))
        e = dict(rows=rows, mu=0.5, f_max=f_max)
        for key, run in (("feet_limited", run_clip), ("qp", run_qp)):
            e[key] = timed(run, runs, lambda: (word.zero_(), count.zero_()))
            st = status[0].cpu().numpy()
            e[key].update(us_per_tick=1e3 * e[key]["median_ms"] / rows, limited_share=float(((st & 256) != 0).mean()), frozen_share=float(((st & 3) != 0).mean()),
                          cap_rows=int(((st & 512) != 0).sum()))
        q = qtable[0].cpu().numpy()
        e["qp"]["steps_mean_of_limited_first_steps"] = float(q[q[:, 0] > 0, 0].mean()) if (q[:, 0] > 0).any() else 0.0
        e["qp"]["steps_most"] = int(q[:, 0].max())
        e["ratio_qp_over_clip"] = e["qp"]["median_ms"] / e["feet_limited"]["median_ms"]
        res[name] = e
        print(name, json.dumps(e), flush=True)

    case("table_256x5001_mu0.5_fmax30", n_all, 30.0, 10)
    case("table_256x5001_mu0.5_fmax16", n_all, 16.0, 10)
    case("tick_256x1", 1, 16.0, 50, first=1234)
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
