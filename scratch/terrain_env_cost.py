"""Cost of a fleet's randomised terrains (DESIGN.md section 6 "Terrain-env kernel", profiles/terrain_env_cost.json): for 1, 16 and 256
copies of the exp_3 map (220 x 660) and of the exp_5 map (220 x 440) at mesh_scale 11, 110 shifts and 10 height passes,
  device  one qtos_terrain_env_device launch (k_terrain_env, one workgroup per map, all maps fanned out from one base grid) and
          qtos_set_heightfields_device behind it, between HIP events on one stream
  host    the route it replaces: heightfield.random_env per map on a random.Random, heightfield.towr_map, and one
          qtos_set_heightfields upload of the stack, host clock
on one handle on the same box, medians behind a warm-up run with the smallest and the largest run next to them, and whether the
two routes leave the same maps.  No speed is gated on these numbers.
Usage: python scratch/terrain_env_cost.py [out.json] [copies,copies,...]"""
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from qtos_amd import capi, heightfield, workloads                        # noqa: E402
from qtos_amd.config import PlannerConfig                                # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "terrain_env_cost.json")
copies = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [1, 16, 256]
RUNS = {1: (50, 10), 16: (20, 5), 256: (10, 3)}                          # copies -> (device runs, host runs)
SCALE, N_SHIFT, N_HEIGHT = 11, 110, 10
dev = torch.device("cuda", 0)
P = capi.Planner(PlannerConfig.reference_compat(), max_batch=4)
st = torch.cuda.current_stream(dev)
sp = C.c_void_p(st.cuda_stream)
med = statistics.median
rows = []
for name, tiles, climb in (("exp_3", ("feasibility_test", "feasibility_test_1", "plane"), False), ("exp_5", ("climb_2", "climb_1"), True)):
    base = heightfield.build_map([workloads.tile(t) for t in tiles], SCALE)
    r, c = base.shape
    cell = heightfield.cell_size(base)
    d_base = torch.as_tensor(base[None], dtype=torch.float64, device=dev)
    for n in copies:
        dev_runs, host_runs = RUNS.get(n, (3, 1))
        seeds = list(range(1000, 1000 + n))
        d_seed = torch.as_tensor(np.array(seeds, np.int64), device=dev)
        d_bid = torch.zeros(n, dtype=torch.int32, device=dev)
        d_map, d_hxy = torch.zeros((n, r, c), dtype=torch.float64, device=dev), torch.zeros((n, c, r), dtype=torch.float64, device=dev)
        d_status = torch.zeros(n, dtype=torch.int32, device=dev)
        g = capi.terrain_env_params((1, r, c), n, N_SHIFT, N_HEIGHT, climb)
        dev_ms, kernel_ms = [], []
        for i in range(1 + dev_runs):                                    # (the first run is the warm-up)
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            torch.cuda.synchronize()
            e0.record(st)
            rc = P.lib.qtos_terrain_env_device(P.h, C.byref(g), d_base.data_ptr(), d_bid.data_ptr(), d_seed.data_ptr(), None, d_map.data_ptr(),
                                               d_hxy.data_ptr(), d_status.data_ptr(), sp)
            e1.record(st)
            P.set_heightfields_device(d_hxy, cell, stream=st)
            e2.record(st)
            e2.synchronize()
            assert rc == 0, P.lib.qtos_last_error(P.h)
            if i:
                dev_ms.append(e0.elapsed_time(e2))
                kernel_ms.append(e0.elapsed_time(e1))
        host_ms = []
        for i in range(host_runs):
            torch.cuda.synchronize()
            t = time.perf_counter()
            maps = [heightfield.random_env(base, random.Random(s), N_SHIFT, N_HEIGHT, climb) for s in seeds]
            P.set_heightfields(np.stack([heightfield.towr_map(m) for m in maps]), cell)
            host_ms.append(1e3 * (time.perf_counter() - t))
        got = d_map.cpu().numpy()
        same = all(np.array_equal(got[k].view(np.uint64), maps[k].view(np.uint64)) for k in range(n)) and not d_status.any().item()
        rows.append(dict(map=name, shape=[r, c], copies=n, device_ms_between_events=round(med(dev_ms), 3),
                         device_ms_min_max=[round(min(dev_ms), 3), round(max(dev_ms), 3)], kernel_ms=round(med(kernel_ms), 3), device_runs=dev_runs,
                         host_route_ms=round(med(host_ms), 2), host_ms_min_max=[round(min(host_ms), 2), round(max(host_ms), 2)],
                         host_runs=host_runs, maps_equal=bool(same)))
        print(json.dumps(rows[-1]), flush=True)
        del d_map, d_hxy
res = dict(what="randomised terrains of copies of the exp_3 and exp_5 maps at mesh_scale %d, n_shift %d, n_height %d, seeds 1000 + m, on one "
                "handle; one MI355X" % (SCALE, N_SHIFT, N_HEIGHT),
           device="HIP events around qtos_terrain_env_device (kernel_ms: the launch alone) and qtos_set_heightfields_device on one stream; "
                  "medians behind one warm-up run",
           host="heightfield.random_env per map, towr_map, one qtos_set_heightfields of the stack, host clock; medians", rows=rows)
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
P.close()
