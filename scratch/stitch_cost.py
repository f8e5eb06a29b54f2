"""Cost of keeping the executed trajectory of the receding windows (profiles/stitch_cost.json): bench.py's
mpc_random configuration -- 256 windows in four sets of 64, each set on its own planner, stream and host thread, 200-knot plans,
random terrains -- timed over N replans behind a warm-up, in three alternating passes each of
  a  trajectory=None (what every caller had before)
  b  the ring through k_stitch (ShiftedWindows(trajectory=...))
  c  the ring built the way a caller would build it without k_stitch: qtos_sample_csv_device of k0 + n_search + 1 rows of the
     plan handed over from, then torch indexing into the same ring
and k_stitch alone, from HIP events around single launches on the windows' last plans and hand-over rows.
Usage: python scratch/stitch_cost.py [out.json] [N] [a|abc]      ("a": only pass a, which also runs on a build without k_stitch)"""
import ctypes as C
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qtos_amd import workloads                      # noqa: E402
from qtos_amd.capi import Planner                   # noqa: E402
from qtos_amd.config import PlannerConfig           # noqa: E402
from qtos_amd.replan import ShiftedWindows          # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "stitch_cost.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 50
modes = sys.argv[3] if len(sys.argv) > 3 else "abc"
B, NSET, WARMUP, PASSES, CAP = 256, 4, 5, 3, 8192
per = B // NSET
dev = torch.device("cuda", 0)
rw = PlannerConfig.receding_windows()
cfg = PlannerConfig.knots200(chord_tol=rw.chord_tol, mu_superlinear=rw.mu_superlinear)
terrain = workloads.random_terrains()
start, goal, map_id = workloads.mpc_goals(B, seed=5, terrains=terrain)
gstep = goal - start[:, 0:3]
planners = []
for j in range(NSET):
    P = Planner(cfg, max_batch=per, device=0)
    P.set_heightfields(terrain[0], terrain[1])
    P.set_kernel_events(False)
    planners.append(P)
streams = [torch.cuda.Stream(dev) for _ in range(NSET)]
pool = ThreadPoolExecutor(NSET)


class ByHand:
    """Pass c: the ring of one set without k_stitch -- sample the plan handed over from, scatter its executed rows."""

    def __init__(self, W):
        self.W = W
        self.rows = torch.empty((W.B, int(round(W.advance * W.hz)) + W.n_search + 1, 37), dtype=torch.float64, device=dev)
        self.ring = torch.zeros((W.B, CAP, 37), dtype=torch.float64, device=dev)
        self.cursor = torch.zeros((W.B,), dtype=torch.int64, device=dev)
        self.t0 = torch.zeros((W.B,), dtype=torch.float64, device=dev)
        self.j = torch.arange(self.rows.shape[1], device=dev)[None, :]
        self.base = (torch.arange(W.B, device=dev) * CAP)[:, None]

    def append(self):
        W = self.W                                     # (after replan(): W.prev is the plan handed over from, W.row its hand-over row)
        rc = W.P.lib.qtos_sample_csv_device(W.P.h, W.B, W.prev.data_ptr(), self.t0.data_ptr(), C.c_double(W.hz), self.rows.shape[1],
                                            self.rows.data_ptr(), C.c_void_p(W.stream.cuda_stream))
        assert rc == 0
        n = W.row.to(torch.int64)
        keep = self.j < n[:, None]
        dest = self.base + (self.cursor[:, None] + self.j) % CAP
        self.ring.view(-1, 37)[dest[keep]] = self.rows[keep]
        self.cursor += n
        self.t0 += n.to(torch.float64) / W.hz


def one_pass(mode):
    kw = dict(trajectory=CAP) if mode == "b" else {}
    sets = [ShiftedWindows(planners[j], start[j * per:(j + 1) * per], gstep[j * per:(j + 1) * per], map_id[j * per:(j + 1) * per],
                           advance=2.5, x_range=(0.0, 2.2), stream=streams[j], **kw) for j in range(NSET)]
    hand = [ByHand(W) for W in sets] if mode == "c" else None

    def one(j):
        W = sets[j]
        W.replan()
        if hand is not None and state["replans"] > 0:
            with torch.cuda.stream(W.stream):
                hand[j].append()
        W.stream.synchronize()

    state = {"replans": 0}
    for _ in range(1 + WARMUP):                        # the cold plan and the warm-up
        list(pool.map(one, range(NSET)))
        state["replans"] += 1
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(N):
        list(pool.map(one, range(NSET)))
        state["replans"] += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t
    return B * N / dt, sets, hand


rates = {m: [] for m in modes}
last = {}
for _ in range(PASSES):
    for m in modes:
        r, sets, hand = one_pass(m)
        rates[m].append(r)
        last[m] = (sets, hand)
        print("pass %s: %.0f replans/s" % (m, r), flush=True)
res = dict(what="bench.py's mpc_random configuration (256 windows = 4 sets x 64, knots200, random terrains), %d replans behind a cold plan "
                "and %d warm-up replans, %d alternating passes; one MI355X" % (N, WARMUP, PASSES),
           passes={m: dict(replans_per_s=[round(v, 1) for v in rates[m]], median=round(statistics.median(rates[m]), 1),
                           spread_percent=round(100 * (max(rates[m]) - min(rates[m])) / statistics.median(rates[m]), 2)) for m in modes})
if "b" in modes and "c" in modes:
    # the two rings hold the same rows (same seeds, same plans)
    same = all(torch.equal(W.traj, h.ring) and torch.equal(W.cursor, h.cursor) for W, h in zip(last["b"][0], last["c"][1]))
    res["ring_b_equals_ring_c"] = bool(same)
    print("ring of pass b == ring of pass c:", same)
if "b" in modes:
    # k_stitch alone: single launches between HIP events, a set (64 windows) and all 256 windows at once
    from qtos_amd import capi
    sets = last["b"][0]
    nodes = torch.cat([W.nodes for W in sets]).contiguous()
    row = torch.cat([W.row for W in sets]).contiguous()
    alone = {}
    for nb in (per, B):
        ring = torch.zeros((nb, CAP, 37), dtype=torch.float64, device=dev)
        cur = torch.zeros((nb,), dtype=torch.int64, device=dev)
        t0 = torch.zeros((nb,), dtype=torch.float64, device=dev)
        s = capi.stitch_params(CAP, 0, 0, 1000.0, True)
        st = torch.cuda.current_stream(dev)
        ms = []
        for i in range(25):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            rc = planners[0].lib.qtos_stitch_device(planners[0].h, nb, C.byref(s), nodes.data_ptr(), row.data_ptr(), t0.data_ptr(),
                                                    ring.data_ptr(), cur.data_ptr(), C.c_void_p(st.cuda_stream))
            e1.record(st)
            e1.synchronize()
            assert rc == 0
            if i >= 5:
                ms.append(e0.elapsed_time(e1))
        nbytes = int(row[:nb].to(torch.int64).sum().item()) * 37 * 8
        med = statistics.median(ms)
        alone["%d_windows" % nb] = dict(us_per_launch=round(1e3 * med, 1), us_min=round(1e3 * min(ms), 1), us_max=round(1e3 * max(ms), 1),
                                        rows=nbytes // 296, bytes_written=nbytes, gb_per_s=round(nbytes / (med * 1e-3) / 1e9, 1))
        print("k_stitch alone, %d windows:" % nb, alone["%d_windows" % nb])
    res["k_stitch_alone"] = alone
with open(out, "w") as fh:
    json.dump(res, fh, indent=1)
    fh.write("\n")
for P in planners:
    P.close()
