"""Cost of the boolean maps of a fleet's heightfields (DESIGN.md section 6 "Probe kernels", profiles/probe_cost.json): for 1, 16 and
256 copies of the exp_3 map (20 x 60, 48 probe patches each),
  device  feasibility.feasibility_maps_device -- k_probe, the batched solve in chunks of max_batch, k_probe_stamp -- between HIP
          events, and the host clock around the whole function
  host    the route it replaces: feasibility.feasibility_map once per map (Python loops over the cells, flag dictionaries,
          upload, solve, read back, stamp loop), host clock
on one handle of max_batch 256 on the same box, medians behind a warm-up run with the smallest and the largest run next to them
-- 50 device and 10 host runs for one map, 20 and 5 for 16, 5 and 3 for 256, where a host run takes seconds --, and whether the
two routes leave the same maps.  No speed is gated on these numbers.
Usage: python scratch/probe_cost.py [out.json] [copies,copies,...]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtos_amd import feasibility, heightfield                            # noqa: E402
from qtos_amd.planner import LocalPlanner                                # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "probe_cost.json")
copies = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 16, 256]
RUNS = {1: (50, 10), 16: (20, 5), 256: (5, 3)}                           # copies -> (device runs, host runs)
SHIFT, MAX_BATCH = 3, 256
dev = torch.device("cuda", 0)
tiles = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "data", "heightfields")
tile = lambda name: heightfield.read_tile(os.path.join(tiles, name + ".txt"))
m = heightfield.build_map([tile(n) for n in ("feasibility_test", "feasibility_test_1", "plane")], 1)
lp = LocalPlanner(max_batch=MAX_BATCH)
P = lp.planner()
st = torch.cuda.current_stream(dev)
med = statistics.median
rows = []
for n in copies:
    dev_runs, host_runs = RUNS.get(n, (2, 1))
    maps = np.stack([m] * n)
    lp.set_heightfield(np.stack([heightfield.towr_map(m)] * n), heightfield.cell_size(m))
    d_maps = torch.as_tensor(maps, dtype=torch.float64, device=dev)
    dev_ms, wall_ms = [], []
    for i in range(1 + dev_runs):                                        # (the first run is the warm-up)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t = time.perf_counter()
        e0.record(st)
        bm, offsets, patch, status = feasibility.feasibility_maps_device(P, d_maps, multi_map_shift=SHIFT)
        e1.record(st)
        e1.synchronize()
        if i:
            wall_ms.append(1e3 * (time.perf_counter() - t))
            dev_ms.append(e0.elapsed_time(e1))
    host_ms = []
    for i in range(host_runs):
        torch.cuda.synchronize()
        t = time.perf_counter()
        host = [feasibility.feasibility_map(lp, maps[k], multi_map_shift=SHIFT) for k in range(n)]
        host_ms.append(1e3 * (time.perf_counter() - t))
    same = all(np.array_equal(bm[k].cpu().numpy(), host[k][0].astype(float)) for k in range(n))
    st_dev = status.cpu().numpy()
    rows.append(dict(copies=n, problems=int(offsets[-1].item()), statuses={str(int(k)): int((st_dev == k).sum()) for k in np.unique(st_dev)},
                     device_ms_between_events=round(med(dev_ms), 2), device_ms_min_max=[round(min(dev_ms), 2), round(max(dev_ms), 2)],
                     device_route_host_clock_ms=round(med(wall_ms), 2), device_runs=dev_runs, host_route_ms=round(med(host_ms), 2),
                     host_ms_min_max=[round(min(host_ms), 2), round(max(host_ms), 2)], host_runs=host_runs, maps_equal=bool(same)))
    print(json.dumps(rows[-1]), flush=True)
res = dict(what="boolean maps of copies of the exp_3 map (20 x 60, multi_map_shift 3, 48 probe patches each) on one handle at the default "
                "configuration, max_batch %d; one MI355X" % MAX_BATCH,
           device="feasibility_maps_device: HIP events around the function (k_probe, qtos_plan_batch_device per chunk, k_probe_stamp) and "
                  "the host clock around it; medians behind one warm-up run",
           host="feasibility_map once per map, host clock; medians", rows=rows)
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
lp.close()
