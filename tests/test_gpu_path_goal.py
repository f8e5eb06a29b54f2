"""The path-goal kernel of the receding windows on the MI355X (pytest -m gpu): k_path_goal against the numpy statement of its rule
(global_planner.path_goal) to the bit -- partial workgroups, paths of 1 .. 11 pieces, shared and per-window paths, two height grids
and none, both bases, the clamp, the hold, times before / on / beyond the knots, wrapping and fall-back cells, a NaN clock, every
done bit --, the host form against the device form, the argument checks, the ShiftedWindows loop along two A* paths, and the loop
from plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")

NW = 8                       # windows of the planner the tests share (the kernel's batch is not bound by it)
BMAX = 130
PIECES = (1, 2, 3, 11)
HORIZON, STEP, STOP = 1.0, 0.5, 0.05
PATTERN = -98765.4321


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(a, b):
    """Equal to the bit; a NaN equals a NaN (IEEE leaves its payload open)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


class Spine:
    """What path_table reads of a PathSolver: knots on multiples of 0.25, so that knot - HORIZON + HORIZON is the knot."""

    def __init__(self, n, rng):
        t = np.concatenate([[0.0], np.cumsum(0.25 * rng.integers(4, 13, n))])
        self.spine_x_track = CubicSpline(t, rng.normal(1.0, 1.2, n + 1))       # x, y beyond the grids' -1 .. 3, -1 .. 1 too
        self.spine_y_track = CubicSpline(t, rng.normal(0.0, 0.9, n + 1))
        self.robot_goal = [float(rng.uniform(0.0, 2.0)), 0.0, 0.24]


class Batch:
    """BMAX windows and everything the kernel tests share; a test takes the first B of them (gpu=False: the arrays alone)."""

    def __init__(self, gpu=True):
        from qtos_amd.global_planner import path_goal, path_table
        if gpu:
            import torch
            from qtos_amd.capi import Planner
            from qtos_amd.config import PlannerConfig
            self.torch, self.dev = torch, torch.device("cuda", 0)
            self.P = Planner(PlannerConfig.receding_windows(), max_batch=NW)
        rng = np.random.default_rng(2024)
        spines = [Spine(n, rng) for n in PIECES]
        self.shared = path_table(spines)                                         # 4 paths, chosen through path_id
        self.path_id = (np.arange(BMAX) % 4).astype(np.int32)
        self.own = path_table([spines[b % 4] for b in range(BMAX)])              # path b for window b: path_id NULL
        self.grids = rng.uniform(0.0, 0.1, (2, 20, 40))
        self.map_id = ((np.arange(BMAX) // 2) % 2).astype(np.int32)
        knots, n = self.shared["knots"][self.path_id], self.shared["n_pieces"][self.path_id]
        t_end = knots[np.arange(BMAX), n]
        # plan times lt = clock + offset: random ones from before 0 to beyond the end, then the chosen ones
        lt = rng.uniform(-1.0, t_end + 1.0)
        offset = rng.uniform(0.0, 2.9, BMAX)
        lt[0] = knots[0, 0]                                                      # on the first knot
        lt[1] = np.nan
        for b in range(2, 22):                                                   # tf, then lt exactly on a knot, the last included
            k = (b // 4) % (n[b] + 1)
            lt[b] = knots[b, k] - (HORIZON if b < 12 else 0.0)
        offset[2:34] = 0.25 * (np.arange(2, 34) % 3)                             # (multiples of 0.25: clock + offset is lt exactly)
        lt[22:26] = -7.5                                                         # tf before the first knot
        lt[26:30] = t_end[26:30] + 7.5 + 0.25                                    # bit 0, just
        lt[30:34] = t_end[30:34] + 7.5                                           # not yet: the comparison is strict
        lt[40:52:3] = t_end[40:52:3] + 8.0                                       # both bits (these windows start next to their goals)
        self.offset = offset
        self.clock = lt - offset
        for b in list(range(2, 34)):
            assert self.clock[b] + offset[b] == lt[b]                            # (multiples of 0.25: exact)
        self.done_in = np.where(np.arange(BMAX) % 7 == 3, 4, 0).astype(np.int32)  # bits a window brings along stay
        self.done_in[[5, 27]] = 1
        # start states: random ones near the paths, and from window 40 on every third one next to its goal (bit 1) -- the goal of
        # base "spine" does not depend on the start, and the goal of base "state" from a start at the target is the target
        start = np.zeros((BMAX, 24))
        start[:, 0:3] = rng.uniform([-1.0, -1.0, 0.2], [3.0, 1.0, 0.35], (BMAX, 3))
        start[:, 3:] = rng.standard_normal((BMAX, 21))
        par = self.params("spine", False, False, stop=0.0)
        near = np.arange(40, BMAX, 3)
        self.start = {}
        for base in ("spine", "state"):
            goal, _, _ = path_goal(self.shared, self.path_id, self.grids, self.map_id, self.clock, offset, np.zeros((BMAX, 24)),
                                   dict(par, base=base, step_size=1e9))
            s = start.copy()
            s[near, 0:2] = goal[near, 0:2] + [0.004, -0.003]
            self.start[base] = s
        self.near = near

    def params(self, base, clamp, hold, stop=STOP):
        return dict(horizon=HORIZON, step_size=STEP, tol=1e-5, z_offset=0.24, cell=0.1, origin_x=1.0, origin_y=1.0, t_stop=7.5,
                    stop_dist=stop, base=base, clamp_x=clamp, advance_clock=True, hold_done=hold)

    def struct(self, par, table, grids):
        from qtos_amd import capi
        return capi.path_goal_params(par["horizon"], par["step_size"], par["tol"], par["z_offset"], par["cell"],
                                     (par["origin_x"], par["origin_y"]), par["t_stop"], par["stop_dist"], par["base"], par["clamp_x"],
                                     par["advance_clock"], par["hold_done"], table=table, map_yx=grids)

    def up(self, a, dtype=None):
        torch = self.torch
        if a is None:
            return None
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype or torch.float64, device=self.dev).contiguous()

    def device(self, B, par, table, path_id, grids, map_id, clock, offset, start, done, expect=0):
        """qtos_path_goal_device on copies of the host arrays; returns (goal, done, clock) as numpy."""
        torch = self.torch
        i32 = torch.int32
        t = dict(knots=self.up(table["knots"]), coef=self.up(table["coef"]), n=self.up(table["n_pieces"], i32), rg=self.up(table["robot_goal"]),
                 pid=self.up(path_id, i32), grids=self.up(grids), mid=self.up(map_id, i32), clock=self.up(clock), off=self.up(offset),
                 start=self.up(start), done=self.up(done, i32))
        goal = torch.full((B, 3), PATTERN, dtype=torch.float64, device=self.dev)
        g = self.struct(par, table, grids)
        ptr = lambda x: None if x is None else x.data_ptr()
        torch.cuda.synchronize()
        rc = self.P.lib.qtos_path_goal_device(self.P.h, B, C.byref(g), ptr(t["knots"]), ptr(t["coef"]), ptr(t["n"]), ptr(t["rg"]), ptr(t["pid"]),
                                              ptr(t["grids"]), ptr(t["mid"]), ptr(t["clock"]), ptr(t["off"]), ptr(t["start"]), ptr(goal),
                                              ptr(t["done"]), C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.P.lib.qtos_last_error(self.P.h))
        return goal.cpu().numpy(), None if done is None else t["done"].cpu().numpy(), t["clock"].cpu().numpy()


@pytest.fixture(scope="module")
def batch():
    b = Batch()
    yield b
    b.P.close()


def test_the_batch_holds_the_cases(batch):
    """What the windows were chosen for is in the batch: every kind of time, cell, done bit, and the NaN clock."""
    from qtos_amd.global_planner import _spine_eval_rows, path_goal
    tab, pid = batch.shared, batch.path_id
    knots, n = tab["knots"][pid], tab["n_pieces"][pid]
    lt = batch.clock + batch.offset
    tf = lt + HORIZON
    t_end = knots[np.arange(BMAX), n]
    assert (tf < 0).any() and (lt > t_end).any() and np.isnan(lt[1]) and np.isnan(lt).sum() == 1
    on_knot = lambda t: (knots == t[:, None]).any(axis=1)
    assert on_knot(tf)[2:12].all() and on_knot(lt)[12:22].all() and (tf[2:12] == t_end[2:12]).any() and (lt[12:22] == t_end[12:22]).any()
    for t in (tf, lt):                                           # spine points inside the grids, wrapping, and falling back
        x = _spine_eval_rows(knots, tab["coef"][pid, 0], n, t)
        y = _spine_eval_rows(knots, tab["coef"][pid, 1], n, t)
        fr, fc = np.floor((y + 1.0) / 0.1), np.floor((x + 1.0) / 0.1)
        ok = (fr >= -20) & (fr < 20) & (fc >= -40) & (fc < 40)
        assert (ok & (fr >= 0) & (fc >= 0)).sum() > 10 and (ok & ((fr < 0) | (fc < 0))).sum() > 10 and (~ok).sum() > 10
    for base in ("spine", "state"):
        goal, done, clock = path_goal(tab, pid, batch.grids, batch.map_id, batch.clock, batch.offset, batch.start[base],
                                      batch.params(base, False, False))
        assert {0, 1, 2, 3} <= set(done.tolist()), set(done.tolist())
        assert (done[26:30] & 1).all() and not (done[30:34] & 1).any() and (done[batch.near] & 2).sum() > 10
        moved = np.abs(goal - (batch.start[base][:, 0:3] if base == "state" else goal)).max()
        assert base == "spine" or np.isclose(moved, STEP)                        # (the clip is met)
    goal, _, clock = path_goal(tab, pid, batch.grids, batch.map_id, batch.clock, batch.offset, batch.start["spine"], batch.params("spine", False, False))
    assert np.isnan(goal[1, 0:2]).all() and np.isnan(clock[1])


@pytest.mark.parametrize("B", [1, 63, 65, BMAX])
def test_kernel_is_the_numpy_rule_to_the_bit(batch, B):
    """The NaN clock (window 1): with base "spine" the goal's x and y are NaN -- the spine at a NaN time is NaN and the clip keeps
    it -- and its z is the number the rule gives, as the reference does: get_map_height answers a NaN point with its fall-back cell,
    and the tol rule reads a NaN coordinate as 0.0.  A goal that is NaN in all three components cannot come out of the rule that
    Global_Planner.update is pinned to; the kernel is held to the rule, to the bit, here as everywhere."""
    from qtos_amd.global_planner import path_goal
    cut = lambda a: None if a is None else a[:B]
    n_cases = 0
    for table, path_id in ((batch.shared, batch.path_id), (batch.own, None)):
        for grids, map_id in ((batch.grids, batch.map_id), (batch.grids, None), (None, None)):
            for base in ("spine", "state"):
                for clamp in (False, True):
                    for hold in (False, True):
                        par = batch.params(base, clamp, hold)
                        args = (table, cut(path_id), grids, cut(map_id), batch.clock[:B], batch.offset[:B], batch.start[base][:B])
                        want = path_goal(*args, par, done=batch.done_in[:B])
                        got = batch.device(B, par, *args, batch.done_in[:B])
                        what = (B, path_id is None, grids is None, map_id is None, base, clamp, hold)
                        assert same(got[0], want[0]), (what, np.argwhere(bits(got[0]) != bits(want[0]))[:5])
                        assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1]), what
                        assert same(got[2], want[2]), what
                        if B > 1 and base == "spine":
                            assert np.isnan(got[0][1, 0:2]).all() and np.isfinite(got[0][1, 2]), what
                        if hold:
                            held = want[1] != 0
                            assert np.array_equal(bits(got[0][held]), bits(batch.start[base][:B][held, 0:3])), what
                        n_cases += 1
    # optional arrays left out, and the clock left alone
    par = dict(batch.params("spine", False, False, stop=0.0), advance_clock=False)
    want = path_goal(batch.shared, batch.path_id[:B], None, None, batch.clock[:B], None, None, par)
    got = batch.device(B, par, batch.shared, batch.path_id[:B], None, None, batch.clock[:B], None, None, None)
    assert same(got[0], want[0]) and got[1] is None and same(got[2], batch.clock[:B])
    print("[k_path_goal] B %d: %d parameter sets equal the numpy rule to the bit" % (B, n_cases + 1))


def test_host_form_leaves_what_the_device_form_leaves(batch):
    from qtos_amd.global_planner import path_goal
    B = 65
    for base, clamp, hold, grids in (("spine", True, True, batch.grids), ("state", False, False, None)):
        par = batch.params(base, clamp, hold)
        args = (batch.shared, batch.path_id[:B], grids, None if grids is None else batch.map_id[:B], batch.clock[:B], batch.offset[:B],
                batch.start[base][:B])
        dev = batch.device(B, par, *args, batch.done_in[:B])
        clock0, done0 = batch.clock[:B].copy(), batch.done_in[:B].copy()
        host = batch.P.path_goal(batch.shared, clock0, batch.struct(par, batch.shared, grids), path_id=args[1], map_yx=grids, map_id=args[3],
                                 offset=args[5], start=args[6], done=done0)
        assert same(clock0, batch.clock[:B]) and np.array_equal(done0, batch.done_in[:B])        # (Planner.path_goal returns new arrays)
        assert same(host[0], dev[0]) and np.array_equal(host[1], dev[1]) and same(host[2], dev[2])
        want = path_goal(*args, par, done=batch.done_in[:B])
        assert same(host[0], want[0]) and np.array_equal(host[1], want[1]) and same(host[2], want[2])
    # without done, offset and start; path_id NULL
    par = dict(batch.params("spine", False, False, stop=0.0), advance_clock=False)
    host = batch.P.path_goal(batch.own, batch.clock[:B], batch.struct(par, batch.own, None))
    want = path_goal(batch.own, None, None, None, batch.clock[:B], None, None, par)
    assert same(host[0], want[0]) and host[1] is None and same(host[2], batch.clock[:B])


def test_bad_arguments_answer_minus_one_and_write_nothing(batch):
    from qtos_amd import capi
    torch, P, dev = batch.torch, batch.P, batch.dev
    B = 8
    tab = batch.shared
    good = batch.struct(batch.params("state", True, True), tab, batch.grids)
    i32 = torch.int32
    T = dict(knots=batch.up(tab["knots"]), coef=batch.up(tab["coef"]), n=batch.up(tab["n_pieces"], i32), rg=batch.up(tab["robot_goal"]),
             pid=batch.up(batch.path_id[:B], i32), grids=batch.up(batch.grids), mid=batch.up(batch.map_id[:B], i32),
             clock=batch.up(np.full(B, PATTERN)), off=batch.up(batch.offset[:B]), start=batch.up(batch.start["state"][:B]),
             goal=batch.up(np.full((B, 3), PATTERN)), done=batch.up(np.full(B, 77), i32))
    H = dict(knots=tab["knots"], coef=tab["coef"], n=tab["n_pieces"], rg=tab["robot_goal"], pid=batch.path_id[:B].copy(), grids=batch.grids,
             mid=batch.map_id[:B].copy(), clock=np.full(B, PATTERN), off=batch.offset[:B].copy(), start=batch.start["state"][:B].copy(),
             goal=np.full((B, 3), PATTERN), done=np.full(B, 77, np.int32))
    order = ("knots", "coef", "n", "rg", "pid", "grids", "mid", "clock", "off", "start", "goal", "done")
    ints = ("n", "pid", "mid", "done")

    def device(p=P.h, b=B, g=good, **kw):
        a = [None if k in kw and kw[k] is None else T[k].data_ptr() for k in order]
        return P.lib.qtos_path_goal_device(p, b, None if g is None else C.byref(g), *a, None)

    def host(p=P.h, b=B, g=good, **kw):
        a = [None if k in kw and kw[k] is None else (capi._ip(H[k]) if k in ints else capi._dp(H[k])) for k in order]
        return P.lib.qtos_path_goal(p, b, None if g is None else C.byref(g), *a)

    def params(**kw):
        g = good.copy()
        for k, v in kw.items():
            setattr(g, k, v)
        return g

    torch.cuda.synchronize()
    for name, call in (("device", device), ("host", host)):
        got = {
            "null planner": call(p=None), "B = 0": call(b=0), "B < 0": call(b=-3), "null params": call(g=None),
            "null knots": call(knots=None), "null coef": call(coef=None), "null n_pieces": call(n=None), "null clock": call(clock=None),
            "null goal_out": call(goal=None),
            "n_paths 0": call(g=params(n_paths=0)), "max_pieces 0": call(g=params(max_pieces=0)), "max_pieces < 0": call(g=params(max_pieces=-2)),
            "path_id NULL with n_paths < B": call(pid=None),
            "rows 0 with a grid": call(g=params(rows=0)), "cols < 0 with a grid": call(g=params(cols=-1)), "n_maps 0 with a grid": call(g=params(n_maps=0)),
            "cell 0": call(g=params(cell=0.0)), "cell < 0": call(g=params(cell=-0.1)), "cell NaN": call(g=params(cell=float("nan"))),
            "step_size < 0": call(g=params(step_size=-1e-9)), "base 2": call(g=params(base=2)), "base -1": call(g=params(base=-1)),
            "clamp_x without robot goals": call(rg=None), "hold_done without done": call(done=None),
            "base state without start": call(start=None, g=params(hold_done=0, stop_dist=0.0)),
            "stop_dist without start": call(start=None, g=params(base=0, hold_done=0, stop_dist=0.1)),
            "hold_done without start": call(start=None, g=params(base=0, stop_dist=0.0)),
        }
        assert all(v == -1 for v in got.values()), (name, got)
    torch.cuda.synchronize()
    for name, (goal, clock, done) in (("device", (T["goal"].cpu().numpy(), T["clock"].cpu().numpy(), T["done"].cpu().numpy())),
                                      ("host", (H["goal"], H["clock"], H["done"]))):
        assert (goal == PATTERN).all() and (clock == PATTERN).all() and (done == 77).all(), name
    # on the edge of the checks: accepted (rows / cols are not read without a grid, start not where nothing reads it)
    edge = params(rows=0, cols=0, n_maps=0, base=0, hold_done=0, stop_dist=0.0, step_size=0.0, clamp_x=0)
    for call in (device, host):
        assert call(g=edge, grids=None, mid=None, start=None, rg=None, done=None, off=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(T["goal"].cpu().numpy()), bits(H["goal"])) and not (H["goal"] == PATTERN).any()


# ---- the ShiftedWindows loop along two A* paths ---------------------------------------------------------------------------------

def tile_map(name):
    from qtos_amd import heightfield
    tiles = [heightfield.read_tile(os.path.join(GOLDEN, "heightfields", t + ".txt")) for t in (name, "plane")]
    return heightfield.build_map(tiles, 1)


def submit(P, torch, dev, start, goal, map_id):
    """One cold qtos_plan_submit of a planner with start / goal uploaded from the host; returns (nodes, status, iters)."""
    f64 = dict(dtype=torch.float64, device=dev)
    t_start, t_goal = torch.as_tensor(start, **f64).contiguous(), torch.as_tensor(goal, **f64).contiguous()
    t_map = torch.as_tensor(map_id, dtype=torch.int32, device=dev).contiguous()
    nodes = torch.empty((NW, P.n), **f64)
    status, iters = torch.empty((NW,), dtype=torch.int32, device=dev), torch.empty((NW,), dtype=torch.int32, device=dev)
    viol = torch.empty((NW,), **f64)
    torch.cuda.synchronize()
    rc = P.lib.qtos_plan_submit(P.h, NW, t_start.data_ptr(), t_goal.data_ptr(), t_map.data_ptr(), None, nodes.data_ptr(), status.data_ptr(),
                                iters.data_ptr(), viol.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, P.lib.qtos_last_error(P.h)
    P.wait()
    torch.cuda.synchronize()
    return nodes.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy()


@pytest.mark.parametrize("path_base", ["spine", "state"])
def test_windows_follow_their_paths_and_the_kernel_disturbs_nothing(path_base):
    import torch
    from qtos_amd import heightfield, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import GlobalPlanner, path_goal, path_table
    from qtos_amd.replan import ShiftedWindows
    dev = torch.device("cuda", 0)
    maps_yx = np.stack([tile_map("climb_1"), tile_map("plane")])
    # path 0: A* over climb_1; path 1: a straight path on the plane of 0.8 s -- its end lies t_stop behind the third replan
    gps = [GlobalPlanner(maps_yx[0], [0, 0, 0.24], [2.5, 0.0, 0.24], step_size=1.0), GlobalPlanner(maps_yx[1], [0, 0, 0.24], [0.08, 0.0, 0.24], step_size=1.0)]
    assert all(gp.path_solver.solution_flag for gp in gps) and gps[1].max_t < 1.0 < 20.0 < gps[0].max_t
    table = path_table(gps)
    path_id = np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int32)
    towr = np.stack([heightfield.towr_map(m) for m in maps_yx])                  # the planner's own copy of the terrains: [x][y]
    start = []
    for b in range(NW):
        x, y = 0.02 * b, 0.01 * (b % 3 - 1)
        feet = workloads.NOMINAL_FEET + np.array([x, y, 0.0])
        fz = heightfield.height_at(towr[path_id[b]], 0.1, feet[:, 0], feet[:, 1], mode=1)
        start.append(workloads.rest_start(x, y, 0.24 + float(heightfield.height_at(towr[path_id[b]], 0.1, x, y, mode=1)), fz))
    start = np.stack(start)
    advance = 3.0
    P, P2 = Planner(PlannerConfig.receding_windows(), max_batch=NW), Planner(PlannerConfig.receding_windows(), max_batch=NW)
    try:
        for q in (P, P2):
            q.set_heightfields(towr, 0.1)
        path = dict(table=table, path_id=path_id, map_yx=maps_yx, map_id=path_id, step_size=0.6)
        W = ShiftedWindows(P, start, None, path_id, advance=advance, path=path, path_base=path_base, path_hold=True)
        assert W.goal_step is None and W.clock.dtype == torch.float64 and W.done.dtype == torch.int32
        assert W.path_params.t_stop == 5.0 + advance and W.path_params.horizon == P.dims.duration and W.path_params_init.base == 1
        host = lambda t: t.cpu().numpy().copy()
        clock, done = np.zeros(NW), np.zeros(NW, np.int32)
        held_seen = 0
        for k in range(4):                                                       # the cold plan and three replans
            W.replan()
            torch.cuda.synchronize()
            s, off = host(W.start), host(W.offset) if k else None
            g = W.path_params if k else W.path_params_init
            want_goal, want_done, want_clock = path_goal(table, path_id, maps_yx, path_id, clock, off, s, g, done=done)
            got_goal, got_done, got_clock = host(W.goal), host(W.done), host(W.clock)
            assert same(got_goal, want_goal), (k, np.argwhere(bits(got_goal) != bits(want_goal))[:5])
            assert np.array_equal(got_done, want_done) and np.array_equal(bits(got_clock), bits(want_clock)), k
            held = got_done != 0
            assert np.array_equal(bits(got_goal[held]), bits(s[held, 0:3]))
            held_seen += int(held.sum())
            if k:
                assert ((off >= advance) & (off <= advance + 0.4)).all() and np.array_equal(bits(got_clock), bits(clock + off))
            # a second planner, given the same starts and the goals from the host, returns the same plans: the kernel disturbs nothing
            nodes2, status2, iters2 = submit(P2, torch, dev, s, got_goal, path_id)
            assert np.array_equal(bits(host(W.nodes)), bits(nodes2)), k
            assert np.array_equal(host(W.status), status2) and np.array_equal(host(W.iters), iters2), k
            print("[path loop %s] plan %d: clock %s done %s status %s iters %s goal z %s" % (
                path_base, k, np.round(got_clock, 3).tolist(), got_done.tolist(), status2.tolist(), iters2.tolist(), np.round(got_goal[:, 2], 4).tolist()))
            clock, done = got_clock, got_done
        assert (done[path_id == 1] & 1).all() and not done[path_id == 0].any() and held_seen >= 4        # (the short path's windows have stopped)
    finally:
        P.close()
        P2.close()


def test_c_loop_follows_a_path_for_three_replans(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import path_goal
    from test_path_goal_cpu import two_piece_table
    capi.load()
    exe = tmp_path / "path_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "path_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), str(img)], capture_output=True, text=True, timeout=330)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_path_goal=%d path_goal_null=-1 path_goal_device_null=-1" % C.sizeof(capi.QtosPathGoal)
    assert lines[1] == "bad_args=-1,-1,-1,-1,-1,-1,-1,-1 untouched=1"
    recs = [dict(t.split("=") for t in ln.split()) for ln in lines[2:10]]
    assert [(int(q["replan"]), int(q["window"])) for q in recs] == [(r_, b) for r_ in (0, 1, 2, 3) for b in (0, 1)]
    tab = two_piece_table()
    clock, done = np.array([0.0, 21.0]), np.zeros(2, np.int32)
    par = dict(horizon=5.0, step_size=0.45, tol=1e-5, z_offset=0.24, cell=0.1, origin_x=1.0, origin_y=1.0, t_stop=7.5, stop_dist=0.0,
               clamp_x=False, advance_clock=True, hold_done=True)
    for k in range(4):
        pair = recs[2 * k:2 * k + 2]
        for q in pair:
            assert int(q["handover"]) == 0 and int(q["path_goal"]) == 0 and int(q["plan"]) == 0, q
        start = np.zeros((2, 24))
        start[:, 0:3] = [[float(v) for v in q["start"].split(",")] for q in pair]
        offset = np.array([float(q["offset"]) for q in pair])
        if k:
            assert all(2500 <= int(q["row"]) <= 2900 and float(q["offset"]) == int(q["row"]) / 1000.0 for q in pair), pair
        goal, done, clock = path_goal(tab, np.zeros(2, np.int32), None, None, clock, offset, start, dict(par, base="spine" if k else "state"), done=done)
        got = np.array([[float(v) for v in q["goal"].split(",")] for q in pair])
        assert np.array_equal(bits(got), bits(goal)), (k, got, goal)
        assert [int(q["done"]) for q in pair] == done.tolist() and [float(q["clock"]) for q in pair] == clock.tolist(), pair
    assert done.tolist() == [0, 1] and np.array_equal(got[1], start[1, 0:3])          # (window 1 has passed the path's end and is held)
