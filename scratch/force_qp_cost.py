"""Cost of k_force_qp on one MI355X, between HIP events (not gated; DESIGN.md section 6 "Force-QP kernel"): one launch over 256
windows x 5001 rows of the reference_compat trot, tables and summary, at mu 0.5, at mu 0.2 and at mu 0.5 with a force cap of
16 N, against k_force_fit on the same rows in the same run.  Median of 100 launches after a warm-up, with the smallest and the
largest run.  A wave is as slow as its slowest lane, so next to the share of rows that took the limited path the share of WAVES
(64 consecutive rows of a 128-row tile) with such a row and the mean of the waves' largest step counts are reported: they are
what the time follows.  The float64 numpy route (force_qp.qp_rows) is timed for one window.  Written to the JSON file named on the
command line (profiles/force_qp_cost.json is such a file)."""
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
    from qtos_amd import capi, force_fit as ff, force_qp as fq, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    B, n_all, runs = 256, 5001, 100
    cfg = PlannerConfig.reference_compat(gait="trot")
    P = Planner(cfg, max_batch=B)
    dev = torch.device("cuda", 0)
    x, status, _, _ = P.plan(workloads.rest_start(0.1)[None], np.array([[0.1 + 0.09 * cfg.duration, 0.0, 0.24]]))
    assert status[0] == 0
    f64 = dict(dtype=torch.float64, device=dev)
    nodes = torch.as_tensor(np.repeat(x[:1], B, axis=0), **f64).contiguous()
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
    table = torch.empty((B, n_all, capi.FIT_COLS), **f64)
    qtable = torch.empty((B, n_all, capi.QP_COLS), **f64)
    status = torch.empty((B, n_all), dtype=torch.int32, device=dev)
    summary = torch.as_tensor(ff.empty_summary(B).view(np.float64).reshape(B, 4, 3).copy(), **f64)
    p = capi.fit_params(cfg, n_rows=n_all)
    fit_call = lambda: chk(P.lib.qtos_force_fit_device(P.h, B, C.byref(p), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None, None,
                                                       table.data_ptr(), status.data_ptr(), summary.data_ptr(), sp_))
    res["force_fit"] = timed(fit_call)
    for name, kw in (("mu_0.5", dict(mu=0.5)), ("mu_0.2", dict(mu=0.2)), ("mu_0.5_fmax_16", dict(mu=0.5, f_max=16.0))):
        q = capi.qp_params(cfg, n_rows=n_all, **kw)
        call = lambda: chk(P.lib.qtos_force_qp_device(P.h, B, C.byref(q), nodes.data_ptr(), t0.data_ptr(), None, None, None, None, None, None,
                                                      table.data_ptr(), qtable.data_ptr(), status.data_ptr(), summary.data_ptr(), sp_))
        r = timed(call)
        st, steps = status[0].cpu().numpy(), qtable[0, :, 0].cpu().numpy()
        lim = (st & fq.LIMITED) != 0
        pad = (-n_all) % 64                                                            # (5001 = 39 tiles of 128 and 9 rows: waves of 64 rows)
        per_wave = np.concatenate([lim, np.zeros(pad, bool)]).reshape(-1, 64)
        wave_steps = np.concatenate([steps, np.zeros(pad)]).reshape(-1, 64).max(axis=1)
        r.update(share_rows_limited=float(lim.mean()), share_waves_with_a_limited_row=float(per_wave.any(axis=1).mean()),
                 mean_of_the_waves_largest_step_count=float(wave_steps.mean()), largest_step_count=int(steps.max()),
                 rows_at_the_cap=int(((st & fq.CAP) != 0).sum()), ratio_to_force_fit=r["median_ms"] / res["force_fit"]["median_ms"])
        res["force_qp_" + name] = r
    L = sp.layout(cfg)
    for name, kw in (("mu_0.5", dict(mu=0.5)), ("mu_0.5_fmax_16", dict(mu=0.5, f_max=16.0))):
        ms = []
        for _ in range(3):
            a = time.perf_counter()
            fq.qp_rows(L, x[0], 0.0, 1000.0, 0, n_all, cfg, fq.qp_params(cfg, **kw))
            ms.append(1e3 * (time.perf_counter() - a))
        res["host_numpy_per_window_5001_" + name] = stats(ms)
    print(json.dumps(res, indent=1))
    if out_path:
        json.dump(res, open(out_path, "w"), indent=1)
    P.close()


if __name__ == "__main__":
    main()
