"""Cost of k_rollout_feet next to k_rollout on one MI355X, on the same inputs, between HIP events (not gated; DESIGN.md section 6
"Rollout through the feet"):

  table_256x5001_substeps{1,4}   256 windows x 5001 rows of the golden walk at 1 kHz, tables, joint table given
  ring_256x2500_into_9000        2500 rows per window into rings of 9000 from cursor 8000 (the append wraps)
  tick_256x1                     the one-row tick (the 64-lane instantiation), from the carried state

for both kernels, with the gains of tests/rollout_cases.py on the physical inertia; k_rollout_feet without and with QTOS_FEET_LIMIT.
Median of 50 launches after a warm-up, with the smallest and the largest run; per kernel the time per tick of one window's chain
(median / rows: the windows run side by side, one workgroup each, 256 workgroups on 256 CUs) and the ratio feet / free.  Written to
the JSON file named on the command line (profiles/rollout_feet_cost.json is such a file)."""
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
    from qtos_amd import capi
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

    def chk(rc_):
        assert rc_ == 0, P.lib.qtos_last_error(P.h)

    res = dict(device=torch.cuda.get_device_name(0), windows=B)
    body = dict(cfg=cfg, inertia_b=INERTIA_PHYSICAL, **rc.GAINS)

    def case(name, rows, sub, first=0, capacity=0, cursor0=0, init=True):
        size = capacity if capacity else rows
        joint = torch.zeros((B, size, 37), **f64)
        jp = capi.joint_params(first_row=first, n_rows=rows, capacity=capacity)
        cur = torch.full((B,), cursor0, dtype=torch.int64, device=dev) if capacity else None
        cp = cur.data_ptr() if capacity else None
        jstatus = torch.zeros((B, size), dtype=torch.int32, device=dev)
        chk(P.lib.qtos_joint_rows_device(P.h, B, C.byref(jp), nodes.data_ptr(), t0.data_ptr(), None, None, cp, None, None, joint.data_ptr(),
                                         jstatus.data_ptr(), sp_))
        meas, table, ftable = torch.zeros((B, size, 18), **f64), torch.zeros((B, size, 20), **f64), torch.zeros((B, size, 16), **f64)
        status = torch.zeros((B, size), dtype=torch.int32, device=dev)
        state, count, word = torch.zeros((B, 13), **f64), torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        kw = dict(hz=1000.0, substeps=sub, first_row=first, n_rows=rows, capacity=capacity, init=True, **body)
        free = capi.rollout_params(**kw)
        feet = {False: capi.rollout_feet_params(**kw), True: capi.rollout_feet_params(limit=True, **kw)}
        run_free = lambda: chk(P.lib.qtos_rollout_device(P.h, B, C.byref(free), nodes.data_ptr(), t0.data_ptr(), None, None, cp, joint.data_ptr(), None, None,
                                                         state.data_ptr(), count.data_ptr(), word.data_ptr(), meas.data_ptr(), table.data_ptr(),
                                                         status.data_ptr(), sp_))
        run_feet = lambda lim: chk(P.lib.qtos_rollout_feet_device(P.h, B, C.byref(feet[lim]), nodes.data_ptr(), t0.data_ptr(), None, None, cp, joint.data_ptr(),
                                                                 None, None, state.data_ptr(), count.data_ptr(), word.data_ptr(), meas.data_ptr(),
                                                                 table.data_ptr(), ftable.data_ptr(), status.data_ptr(), sp_))
        e = dict(rows=rows, substeps=sub, free_wrench=timed(run_free), feet=timed(lambda: run_feet(False)), feet_limited=timed(lambda: run_feet(True)))
        for k in ("free_wrench", "feet", "feet_limited"):
            e[k]["us_per_tick"] = 1e3 * e[k]["median_ms"] / rows
        e["ratio_feet_over_free"] = e["feet"]["median_ms"] / e["free_wrench"]["median_ms"]
        e["ratio_limited_over_free"] = e["feet_limited"]["median_ms"] / e["free_wrench"]["median_ms"]
        res[name] = e

    case("table_256x5001_substeps1", n_all, 1)
    case("table_256x5001_substeps4", n_all, 4)
    case("ring_256x2500_into_9000", 2500, 1, capacity=9000, cursor0=8000)
    case("tick_256x1", 1, 1, first=1234)
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
