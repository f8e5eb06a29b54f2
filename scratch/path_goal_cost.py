"""Cost of the goals of the receding windows from their global paths (DESIGN.md section 6 "Path-goal kernel",
profiles/path_goal_cost.json): for B = 256 windows on four A* paths over two height grids,
  device  one qtos_path_goal_device launch (k_path_goal) between HIP events
  host    the route it replaces, per replan: read start / offset back from the device, global_planner.path_goal in numpy, upload
          the goals (and the clock and done bits, which then live on the host)
both as medians of N (>= 50) behind a warm-up, on the same box.  No speed is gated on these numbers.
Usage: python scratch/path_goal_cost.py [out.json] [N]"""
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
from qtos_amd import capi, heightfield                                   # noqa: E402
from qtos_amd.capi import Planner                                        # noqa: E402
from qtos_amd.config import PlannerConfig                                # noqa: E402
from qtos_amd.global_planner import GlobalPlanner, path_goal, path_table  # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "path_goal_cost.json")
N = max(int(sys.argv[2]) if len(sys.argv) > 2 else 100, 50)
B, WARMUP = 256, 10
dev = torch.device("cuda", 0)
tiles = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "data", "heightfields")
tile = lambda name: heightfield.read_tile(os.path.join(tiles, name + ".txt"))
maps = np.stack([heightfield.build_map([tile("climb_1"), tile("plane")], 1), heightfield.build_map([tile("plane"), tile("plane")], 1)])
gps = [GlobalPlanner(maps[m], [0, 0, 0.24], goal, step_size=1.0) for m, goal in ((0, [2.5, 0.0, 0.24]), (0, [1.5, 0.4, 0.24]),
                                                                                 (1, [2.5, 0.3, 0.24]), (1, [0.8, -0.3, 0.24]))]
table = path_table(gps)
rng = np.random.default_rng(1)
path_id = rng.integers(0, len(gps), B).astype(np.int32)
map_id = (path_id // 2).astype(np.int32)
clock = rng.uniform(0.0, 20.0, B)
offset = rng.uniform(2.5, 2.9, B)
start = np.zeros((B, 24))
start[:, 0:3] = rng.uniform([0.0, -0.4, 0.24], [2.5, 0.4, 0.32], (B, 3))
P = Planner(PlannerConfig.receding_windows(), max_batch=8, device=0)
params = capi.path_goal_params(horizon=P.dims.duration, step_size=0.6, t_stop=7.5, base="spine", advance_clock=False, hold_done=True,
                               table=table, map_yx=maps)
f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
up = lambda a, kw: torch.as_tensor(np.ascontiguousarray(a), **kw).contiguous()
T = dict(knots=up(table["knots"], f64), coef=up(table["coef"], f64), n=up(table["n_pieces"], i32), rg=up(table["robot_goal"], f64),
         pid=up(path_id, i32), grids=up(maps, f64), mid=up(map_id, i32), clock=up(clock, f64), off=up(offset, f64), start=up(start, f64),
         goal=torch.zeros((B, 3), **f64), done=torch.zeros((B,), **i32))
st = torch.cuda.current_stream(dev)


def launch():
    rc = P.lib.qtos_path_goal_device(P.h, B, C.byref(params), T["knots"].data_ptr(), T["coef"].data_ptr(), T["n"].data_ptr(),
                                     T["rg"].data_ptr(), T["pid"].data_ptr(), T["grids"].data_ptr(), T["mid"].data_ptr(),
                                     T["clock"].data_ptr(), T["off"].data_ptr(), T["start"].data_ptr(), T["goal"].data_ptr(),
                                     T["done"].data_ptr(), C.c_void_p(st.cuda_stream))
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
kernel_goal, kernel_done = T["goal"].cpu().numpy(), T["done"].cpu().numpy()

host_us, done_h = [], np.zeros(B, np.int32)
for i in range(WARMUP + N):
    torch.cuda.synchronize()
    t = time.perf_counter()
    s, off = T["start"].cpu().numpy(), T["off"].cpu().numpy()                      # read back
    goal, _, _ = path_goal(table, path_id, maps, map_id, clock, off, s, params, done=done_h)
    T["goal"].copy_(torch.from_numpy(goal))                                        # upload
    torch.cuda.synchronize()
    if i >= WARMUP:
        host_us.append(1e6 * (time.perf_counter() - t))
equal = bool(np.array_equal(goal.view(np.int64), kernel_goal.view(np.int64)))

med = statistics.median
res = dict(what="goals of %d receding windows from 4 A* paths (%d pieces at most) over 2 height grids of 20 x 40; medians of %d behind "
                "%d warm-up runs; one MI355X" % (B, table["coef"].shape[3], N, WARMUP),
           device=dict(us_per_launch=round(med(device_us), 1), us_min=round(min(device_us), 1), us_max=round(max(device_us), 1),
                       how="HIP events around one qtos_path_goal_device launch"),
           host=dict(us_per_replan=round(med(host_us), 1), us_min=round(min(host_us), 1), us_max=round(max(host_us), 1),
                     how="read start / offset back, global_planner.path_goal in numpy, upload the goals; host clock around the three"),
           goals_equal_to_the_bit=equal, done_windows=int((kernel_done != 0).sum()))
print(json.dumps(res, indent=1))
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
P.close()
