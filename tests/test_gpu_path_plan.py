"""The path-plan kernel of the receding windows on the MI355X (pytest -m gpu): k_path_plan against the numpy statement of its rule
(global_planner.path_plan) to the bit -- cells, lengths, statuses, knots, coefficients, piece counts and done bits of one batch of
11 windows over 3 maps that holds every case (tests/test_path_plan_cpu.py builds and checks it) --, a call without cells and done
bits, the host form, the argument checks, the ShiftedWindows loop with paths planned on the device and planned anew, and the
caller in plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_path_plan_cpu import (BATCH_PARAMS, BATCH_STATUS, FIT_GATE, batch_arrays, bits, same, tile_map)

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
NW = 4
PATTERN, IPATTERN = -98765.4321, -77
OUT_F, OUT_I = ("knots", "coef"), ("n_pieces", "cells", "n_cells", "status")


@pytest.fixture(scope="module")
def gpu():
    import torch
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    P = Planner(PlannerConfig.receding_windows(), max_batch=NW)
    yield torch, torch.device("cuda", 0), P
    P.close()


@pytest.fixture(scope="module")
def want():
    """The numpy rule on the batch, once."""
    from qtos_amd.global_planner import path_plan
    maps, map_id, start, goal, done = batch_arrays()
    out = path_plan(maps, map_id, start, goal, BATCH_PARAMS, done=done)
    assert out["status"].tolist() == BATCH_STATUS
    return out


def device_call(gpu, g, cells=True, done=True, B=None, **swap):
    """qtos_path_plan_device on the batch with pattern-filled outputs; returns (rc, outputs as numpy)."""
    torch, dev, P = gpu
    maps, map_id, start, goal, done_in = batch_arrays()
    B = len(start) if B is None else B
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    mp, mc = BATCH_PARAMS["max_pieces"], BATCH_PARAMS["max_cells"]
    T = dict(maps=torch.as_tensor(maps, **f64), map_id=torch.as_tensor(map_id, **i32), start=torch.as_tensor(start, **f64),
             goal=torch.as_tensor(goal, **f64), knots=torch.full((len(start), mp + 1), PATTERN, **f64),
             coef=torch.full((len(start), 2, 4, mp), PATTERN, **f64), n_pieces=torch.full((len(start),), IPATTERN, **i32),
             cells=torch.full((len(start), mc, 2), IPATTERN, **i32), n_cells=torch.full((len(start),), IPATTERN, **i32),
             status=torch.full((len(start),), IPATTERN, **i32), done=torch.as_tensor(done_in, **i32))
    ptr = {k: v.data_ptr() for k, v in T.items()}
    if not cells:
        ptr["cells"] = None
    if not done:
        ptr["done"] = None
    ptr.update(swap)
    torch.cuda.synchronize()
    rc = P.lib.qtos_path_plan_device(P.h, B, C.byref(g), ptr["maps"], ptr["map_id"], ptr["start"], ptr["goal"], ptr["knots"], ptr["coef"],
                                     ptr["n_pieces"], ptr["cells"], ptr["n_cells"], ptr["status"], ptr["done"],
                                     C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in T.items()}


def batch_params(**kw):
    from qtos_amd import capi
    maps = batch_arrays()[0]
    par = dict(BATCH_PARAMS, **kw)
    return capi.path_plan_params(step_size=par["step_size"], cell=par["cell"], origin=(par["origin_x"], par["origin_y"]),
                                 height_bound=par["height_bound"], max_cells=par["max_cells"], max_open=par["max_open"],
                                 max_pieces=par["max_pieces"], set_done=par["set_done"], bool_map=maps)


def assert_equal_to_the_bit(got, want, keys_f=OUT_F, keys_i=OUT_I):
    for k in keys_i:
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:5].tolist())
    for k in keys_f:
        assert same(got[k], want[k]), (k, np.argwhere(bits(got[k]) != bits(want[k]))[:5].tolist())


def test_kernel_is_the_numpy_rule_to_the_bit(gpu, want):
    rc, got = device_call(gpu, batch_params())
    assert rc == 0, gpu[2].lib.qtos_last_error(gpu[2].h)
    print("status %s n_cells %s n_pieces %s done %s" % (got["status"].tolist(), got["n_cells"].tolist(), got["n_pieces"].tolist(),
                                                        got["done"].tolist()))
    assert_equal_to_the_bit(got, want)
    assert np.array_equal(got["done"], want["done"]) and got["done"].tolist() == [0, 1, 0, 2, 0, 0, 4, 5, 4, 6, 0]
    inputs = batch_arrays()
    assert same(got["start"], inputs[2]) and same(got["goal"], inputs[3])       # (the inputs stay)


def test_a_call_without_cells_and_done_bits(gpu, want):
    rc, got = device_call(gpu, batch_params(set_done=False), cells=False, done=False)
    assert rc == 0, gpu[2].lib.qtos_last_error(gpu[2].h)
    assert_equal_to_the_bit(got, want, keys_i=("n_pieces", "n_cells", "status"))
    assert (got["cells"] == IPATTERN).all() and np.array_equal(got["done"], batch_arrays()[4])
    # and the first B windows alone, without their map ids: every window on map 0
    from qtos_amd.global_planner import path_plan
    maps, _, start, goal, done = batch_arrays()
    rc, part = device_call(gpu, batch_params(), B=5, map_id=None)
    assert rc == 0
    sub = path_plan(maps, None, start[:5], goal[:5], BATCH_PARAMS, done=done[:5])
    for k in OUT_I + OUT_F:
        a, b = part[k][:5], sub[k]
        assert np.array_equal(a, b) if a.dtype == np.int32 else same(a, b), k
        assert (part[k][5:] == (IPATTERN if a.dtype == np.int32 else PATTERN)).all(), k


def test_host_form_leaves_what_the_device_form_leaves(gpu, want):
    P = gpu[2]
    maps, map_id, start, goal, done = batch_arrays()
    out = P.path_plan(maps, start, goal, batch_params(), map_id=map_id, done=done)
    assert_equal_to_the_bit(out, want)
    assert np.array_equal(out["done"], want["done"]) and same(out["robot_goal"], goal)
    bare = P.path_plan(maps, start[:, 0:2], goal, batch_params(set_done=False), map_id=map_id, cells=False)
    assert bare["cells"] is None and "done" not in bare
    assert_equal_to_the_bit(bare, want, keys_i=("n_pieces", "n_cells", "status"))


def test_bad_arguments_answer_minus_two_and_launch_nothing(gpu):
    P = gpu[2]
    bad = [dict(max_open=4097), dict(max_open=0), dict(max_cells=49), dict(max_cells=0), dict(max_pieces=0, max_cells=0), dict(cell=0.0),
           dict(cell=float("nan")), dict(step_size=0.0), dict(height_bound=float("nan"))]
    calls = [(batch_params(**kw), {}) for kw in bad]
    g = batch_params()
    g.rows, g.cols = 129, 128                                                  # rows * cols > 16384
    calls.append((g, {}))
    g = batch_params()
    g.n_maps = 0
    calls.append((g, {}))
    calls += [(batch_params(), dict(B=0)), (batch_params(), dict(done=False)), (batch_params(), dict(status=None)),
              (batch_params(), dict(n_cells=None)), (batch_params(), dict(maps=None)), (batch_params(), dict(start=None)),
              (batch_params(), dict(goal=None)), (batch_params(), dict(knots=None)), (batch_params(), dict(coef=None)),
              (batch_params(), dict(n_pieces=None))]
    for g, kw in calls:
        rc, got = device_call(gpu, g, **kw)
        assert rc == -2, (rc, kw)
        assert b"qtos_path_plan" in P.lib.qtos_last_error(P.h)
        assert all((got[k] == PATTERN).all() for k in OUT_F) and all((got[k] == IPATTERN).all() for k in OUT_I)
        assert np.array_equal(got["done"], batch_arrays()[4])
    with pytest.raises(RuntimeError):
        maps, map_id, start, goal, done = batch_arrays()
        P.path_plan(maps, start, goal, batch_params(max_open=5000), map_id=map_id)


# ---- the ShiftedWindows loop with paths planned on the device -------------------------------------------------------------------

def test_windows_plan_their_paths_on_the_device_and_plan_them_anew():
    import torch
    from qtos_amd import heightfield, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import GlobalPlanner, path_goal, path_plan, path_table
    from qtos_amd.replan import ShiftedWindows
    grid = tile_map("feasibility_test")
    towr = heightfield.towr_map(grid)[None]
    robot_goal = np.array([[2.5, 0.5, 0.24], [2.5, 0.0, 0.24], [1.5, 0.0, 0.24], [2.7, -0.6, 0.24]])
    start = []
    for b in range(NW):
        x, y = 0.02 * b, 0.01 * (b % 3 - 1)
        feet = workloads.NOMINAL_FEET + np.array([x, y, 0.0])
        fz = heightfield.height_at(towr[0], 0.1, feet[:, 0], feet[:, 1], mode=1)
        start.append(workloads.rest_start(x, y, 0.24 + float(heightfield.height_at(towr[0], 0.1, x, y, mode=1)), fz))
    start = np.stack(start)
    step = 0.6
    gps = [GlobalPlanner(grid, start[b, 0:3], robot_goal[b], step_size=step) for b in range(NW)]
    assert all(gp.path_solver.solution_flag for gp in gps)
    scipy_table = path_table(gps)
    P = Planner(PlannerConfig.receding_windows(), max_batch=NW)
    host = lambda t: t.cpu().numpy().copy()
    try:
        P.set_heightfields(towr, 0.1)
        plan = dict(bool_map=grid, robot_goal=robot_goal, max_pieces=32)
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, None, None, path=dict(plan=plan, table=scipy_table, step_size=step))
        W = ShiftedWindows(P, start, None, np.zeros(NW, np.int32), advance=3.0, path=dict(plan=plan, map_yx=grid, step_size=step))
        par = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=step, max_cells=64, max_open=4096, max_pieces=32,
                   set_done=True)
        assert (W._path_plan_params.max_cells, W._path_plan_params.max_pieces, W._path_plan_params.set_done) == (64, 32, 1)

        def table_of(W, start_xy, goals):
            """The table on the device, which is the numpy rule's to the bit."""
            torch.cuda.synchronize()
            tab = dict(knots=host(W._path_knots), coef=host(W._path_coef), n_pieces=host(W._path_n), robot_goal=host(W._path_rg))
            rule = path_plan(grid, None, start_xy, goals, par, done=np.zeros(NW, np.int32))
            for k in ("knots", "coef", "robot_goal"):
                assert same(tab[k], rule[k]), k
            assert np.array_equal(tab["n_pieces"], rule["n_pieces"]) and np.array_equal(host(W.path_status), rule["status"])
            assert np.array_equal(host(W.path_cells), rule["cells"]) and np.array_equal(host(W.path_n_cells), rule["n_cells"])
            return tab

        table = table_of(W, start, robot_goal)
        assert not host(W.path_status).any() and np.array_equal(table["n_pieces"], scipy_table["n_pieces"])
        assert W.path_status.dtype == torch.int32 and not host(W.done).any() and not host(W.clock).any()
        clock, done = np.zeros(NW), np.zeros(NW, np.int32)
        for k in range(4):                                                      # the cold plan and three replans
            W.replan()
            torch.cuda.synchronize()
            s, off = host(W.start), host(W.offset) if k else None
            g = W.path_params if k else W.path_params_init
            want_goal, want_done, want_clock = path_goal(table, None, grid, None, clock, off, s, g, done=done)
            got_goal = host(W.goal)
            assert same(got_goal, want_goal), (k, got_goal, want_goal)
            assert np.array_equal(host(W.done), want_done) and np.array_equal(bits(host(W.clock)), bits(want_clock)), k
            ref_goal, _, _ = path_goal(scipy_table, None, grid, None, clock, off, s, g, done=done)
            diff = np.abs(got_goal - ref_goal).max()
            print("[plan loop] plan %d: clock %s goal %s |goal - scipy's| %.3g status %s" % (
                k, np.round(want_clock, 3).tolist(), np.round(got_goal[:, 0:2], 4).tolist(), diff, host(W.status).tolist()))
            assert diff <= FIT_GATE * (k + 1) * max(1.0, np.abs(ref_goal).max()), (k, diff)
            clock, done = want_clock, want_done
        assert clock.min() > 8.9
        # new goals: the paths are planned anew from where the windows stand, the clock starts again
        new_goal = robot_goal[::-1].copy()
        W.begin()
        with pytest.raises(RuntimeError):
            W.repath(new_goal)                                                  # refused while a replan is pending
        P.wait()
        assert W.poll()
        W.repath(robot_goal=new_goal)
        torch.cuda.synchronize()
        assert not host(W.clock).any() and not host(W.done).any()
        s = host(W.start)
        table2 = table_of(W, s[:, 0:2], new_goal)
        assert not same(table2["coef"], table["coef"])
        W.replan()
        torch.cuda.synchronize()
        s, off = host(W.start), host(W.offset)
        want_goal, want_done, want_clock = path_goal(table2, None, grid, None, np.zeros(NW), off, s, W.path_params, done=np.zeros(NW, np.int32))
        assert same(host(W.goal), want_goal) and np.array_equal(bits(host(W.clock)), bits(off)) and np.array_equal(host(W.done), want_done)
        # a goal beyond the map has no path: status 1, bit 2, and the window is held on its start
        W.repath(robot_goal=np.array([[4.7, -0.6, 0.24]] * NW))
        W.replan()
        torch.cuda.synchronize()
        assert host(W.path_status).tolist() == [1] * NW and host(W.done).tolist() == [4] * NW
        assert same(host(W.goal), host(W.start)[:, 0:3])
    finally:
        P.close()


def test_c_caller_plans_paths_and_takes_a_step(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import path_goal, path_plan
    capi.load()
    exe = tmp_path / "pathplan_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "pathplan_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout[:2000], r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_path_plan=%d path_plan_null=-1 path_plan_device_null=-1" % C.sizeof(capi.QtosPathPlan)
    assert lines[1] == "bad_args=-2,-2,-2,-2,-2,-2,-2,-2,-2 untouched=1 reason=1"
    recs = [dict(t.split("=") for t in ln.split()) for ln in lines[2:5]]
    grid = np.zeros((10, 16))
    grid[1:8, 7] = 1.0
    start = np.zeros((3, 24))
    start[:, 0:3] = [[-0.85, -0.55, 0.24], [-0.85, -0.95, 0.24], [-0.85, -0.55, 0.24]]
    goals = np.array([[0.45, -0.45, 0.24], [0.45, -0.95, 0.24], [1.45, -0.45, 0.24]])
    par = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=0.25, max_cells=40, max_open=256, max_pieces=20, set_done=True)
    tab = path_plan(grid, None, start, goals, par, done=np.zeros(3, np.int32))
    assert tab["status"].tolist() == [0, 0, 1] and tab["n_cells"][1] == 14 and tab["n_cells"][0] > 14
    step = dict(horizon=5.0, step_size=0.25, tol=1e-5, z_offset=0.24, cell=0.1, origin_x=1.0, origin_y=1.0, t_stop=7.5, stop_dist=0.0,
                base="state", clamp_x=True, advance_clock=True, hold_done=True)
    goal, done, _ = path_goal(tab, None, None, None, np.zeros(3), None, start, step, done=tab["done"])
    nums = lambda q, key, kind: np.array([kind(v) for v in q[key].split(",")])
    for b, q in enumerate(recs):
        assert (int(q["window"]), int(q["path_plan"]), int(q["path_goal"])) == (b, 0, 0)
        assert (int(q["status"]), int(q["n_cells"]), int(q["n_pieces"]), int(q["done"])) == (tab["status"][b], tab["n_cells"][b], tab["n_pieces"][b], done[b])
        assert same(nums(q, "knots", float), tab["knots"][b]) and same(nums(q, "coef", float), tab["coef"][b].ravel())
        assert np.array_equal(nums(q, "cells", int), tab["cells"][b].ravel())
        assert same(nums(q, "goal", float), goal[b])
    assert done.tolist() == [0, 0, 4] and same(goal[2], start[2, 0:3])          # (no path: held on its start)
