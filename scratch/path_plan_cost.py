"""Cost of the global paths of the receding windows (DESIGN.md section 6 "Path-plan kernel", profiles/path_plan_cost.json): for
B = 256 windows on the five 20 x 40 golden maps,
  device  one qtos_path_plan_device launch (k_path_plan) between HIP events, median of N (>= 50) behind a warm-up
  host    the route it replaces: 256 x PathSolver (A* and two scipy CubicSplines each), path_table, upload of the table; host clock
          around the three, median of 5 runs
on the same box, plus how far the table is from scipy's (the measure of tests/test_path_plan_cpu.py fit_error) and whether the
kernel's table equals the numpy rule's to the bit.  No speed is gated on these numbers.
Usage: python scratch/path_plan_cost.py [out.json] [N]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from qtos_amd import capi, heightfield                                   # noqa: E402
from qtos_amd.capi import Planner                                        # noqa: E402
from qtos_amd.config import PlannerConfig                                # noqa: E402
from qtos_amd.global_planner import PathSolver, path_plan, path_table    # noqa: E402
from test_path_plan_cpu import FIT_GATE, FIT_MEASURED, fit_error         # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "path_plan_cost.json")
N = max(int(sys.argv[2]) if len(sys.argv) > 2 else 100, 50)
B, WARMUP, HOST_RUNS = 256, 10, 5
dev = torch.device("cuda", 0)
tiles = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "data", "heightfields")
tile = lambda name: heightfield.read_tile(os.path.join(tiles, name + ".txt"))
names = ("plane", "climb_1", "climb_2", "feasibility_test", "feasibility_test_1")
maps = np.stack([heightfield.build_map([tile(n), tile("plane")], 1) for n in names])
rng = np.random.default_rng(1)
map_id = (np.arange(B) % len(names)).astype(np.int32)
start = np.zeros((B, 24))
start[:, 0:3] = np.column_stack([rng.uniform(-0.2, 0.2, B), rng.uniform(-0.3, 0.3, B), np.full(B, 0.24)])
goal = np.column_stack([rng.uniform(1.2, 2.8, B), rng.uniform(-0.7, 0.7, B), np.full(B, 0.24)])
STEP = 1.0

P = Planner(PlannerConfig.receding_windows(), max_batch=8, device=0)
g = capi.path_plan_params(step_size=STEP, max_pieces=64, bool_map=maps)
f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
up = lambda a, kw: torch.as_tensor(np.ascontiguousarray(a), **kw).contiguous()
mp, mc = int(g.max_pieces), int(g.max_cells)
T = dict(maps=up(maps, f64), mid=up(map_id, i32), start=up(start, f64), rg=up(goal, f64), knots=torch.zeros((B, mp + 1), **f64),
         coef=torch.zeros((B, 2, 4, mp), **f64), n=torch.zeros((B,), **i32), cells=torch.zeros((B, mc, 2), **i32),
         nc=torch.zeros((B,), **i32), status=torch.zeros((B,), **i32))
st = torch.cuda.current_stream(dev)


def launch():
    rc = P.lib.qtos_path_plan_device(P.h, B, C.byref(g), T["maps"].data_ptr(), T["mid"].data_ptr(), T["start"].data_ptr(), T["rg"].data_ptr(),
                                     T["knots"].data_ptr(), T["coef"].data_ptr(), T["n"].data_ptr(), T["cells"].data_ptr(),
                                     T["nc"].data_ptr(), T["status"].data_ptr(), None, C.c_void_p(st.cuda_stream))
    assert rc == 0, P.lib.qtos_last_error(P.h)


device_us = []
for i in range(WARMUP + N):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(st)
    launch()
    e1.record(st)
    e1.synchronize()
    if i >= WARMUP:
        device_us.append(1e3 * e0.elapsed_time(e1))
kernel = {k: T[k].cpu().numpy() for k in ("knots", "coef", "n", "cells", "nc", "status")}

host_ms = []
for i in range(HOST_RUNS):
    torch.cuda.synchronize()
    t = time.perf_counter()
    solvers = [PathSolver(maps[map_id[b]], start[b, 0:3], goal[b], step_size=STEP) for b in range(B)]
    found = [s for s in solvers if s.solution_flag]
    table = path_table(found)
    tabs = [up(table[k], f64) for k in ("knots", "coef", "robot_goal")] + [up(table["n_pieces"], i32)]
    torch.cuda.synchronize()
    host_ms.append(1e3 * (time.perf_counter() - t))

rule = path_plan(maps, map_id, start, goal, g)
equal = all(np.array_equal(kernel[a].view(np.int64) if kernel[a].dtype == np.float64 else kernel[a],
                           rule[b].view(np.int64) if rule[b].dtype == np.float64 else rule[b])
            for a, b in (("knots", "knots"), ("coef", "coef"), ("n", "n_pieces"), ("cells", "cells"), ("nc", "n_cells"), ("status", "status")))
ok = np.flatnonzero(kernel["status"] == 0)
assert [bool(s.solution_flag) for s in solvers] == (kernel["status"] == 0).tolist()
worst = max(fit_error(kernel["coef"][b, a, :, :kernel["n"][b]], getattr(solvers[b], ("spine_x_track", "spine_y_track")[a]).c)
            for b in ok for a in (0, 1))

med = statistics.median
res = dict(what="global paths of %d receding windows over the five 20 x 40 golden maps (%d found, %d .. %d cells, %d pieces at most); one "
                "MI355X" % (B, len(ok), kernel["nc"][ok].min(), kernel["nc"][ok].max(), kernel["n"][ok].max()),
           device=dict(us_per_launch=round(med(device_us), 1), us_min=round(min(device_us), 1), us_max=round(max(device_us), 1),
                       how="HIP events around one qtos_path_plan_device launch, median of %d behind %d warm-up runs" % (N, WARMUP)),
           host=dict(ms_per_run=round(med(host_ms), 1), ms_min=round(min(host_ms), 1), ms_max=round(max(host_ms), 1),
                     how="256 x PathSolver, path_table, upload of the table; host clock around the three, median of %d runs" % HOST_RUNS),
           table_equals_numpy_rule_to_the_bit=bool(equal),
           spine_fit_against_scipy=dict(these_paths=float("%.3g" % worst), cpu_sweep_measured=FIT_MEASURED, gate=FIT_GATE,
                                        measure="largest |difference| of a coefficient row over the row's largest |c| (fit_error)"))
print(json.dumps(res, indent=1))
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
P.close()
