"""The global paths of receding windows without a GPU: the numpy statement of k_path_plan's rule (global_planner.path_cells,
spine_fit, path_plan) against PathSolver.astar, which is pinned to the reference, cell for cell, against scipy's CubicSpline within
a measured gate, and against path_table of the GlobalPlanner; the C ABI of qtos_path_plan*, the C99 caller's build and argument
checks, and the resources of k_path_plan read from the gfx950 code object.  The batch of windows that the GPU test runs
(tests/test_gpu_path_plan.py) is built and checked here."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_path_goal_cpu import REF, bits, same, tile_map  # noqa: E402
from test_stitch_cpu import CSRC, field, notes, one_kernel  # noqa: E402,F401  (the code object's notes, read as that file reads them)

GOLDEN_MAPS = ("plane", "climb_1", "climb_2", "feasibility_test", "feasibility_test_1")
GOLDEN_GOALS = ((1.5, 0.0), (2.5, 0.5), (2.7, -0.6), (4.7, -0.6))
# spine_fit against scipy's CubicSpline.c: the worst fit_error over the sweep of test_spine_fit_is_cubic_spline_within_the_gate,
# measured on the CPU (scipy 1.15.3 with its bundled LAPACK: 6.9e-15), and the gate at 8 x that -- the margin for another LAPACK
# or libm build.  Both solve the same well-conditioned system; they differ in the order of the elimination alone.
FIT_MEASURED = 6.9e-15
FIT_GATE = 8 * FIT_MEASURED
LDS_BYTES = 139264            # DESIGN.md 6, "Path-plan kernel": 16384 x 4 + 16384 x 2 + 4096 x 8 + 4096 x 2


def fit_error(c, w):
    """The difference of two coefficient tables [4, n] over the row's largest |c|, per row of c (one power of t - x[i]); a
    row above the curve's degree (n = 1: the line, n = 2: the parabola) is zero but for rounding, and is held against the largest
    |c| of the whole spline."""
    n = w.shape[1]
    worst = 0.0
    for k in range(4):
        den = np.abs(w[k]).max() if k >= 3 - min(n, 3) else np.abs(w).max()
        err = np.abs(c[k] - w[k]).max()
        if err > 0:
            worst = max(worst, err / den)
    return worst


def astar_reference(bool_map, start, goal):
    """PathSolver.astar alone (the spline fit of a full PathSolver needs a path)."""
    from qtos_amd.global_planner import PathSolver
    ps = PathSolver.__new__(PathSolver)
    ps.bool_map = np.asarray(bool_map)
    ps.solution_flag = False
    ps.grid_res, ps.origin_x_shift, ps.origin_y_shift = 0.1, 1.0, 1.0
    return ps.astar(ps.convert_2_idx(*start), ps.convert_2_idx(*goal))


def open_need(m, s, g):
    """The smallest max_open with which the search of this case does not meet the cap."""
    from qtos_amd.global_planner import path_cells
    lo, hi = 1, 4096
    while lo < hi:
        mid = (lo + hi) // 2
        if path_cells(m, s, g, max_open=mid)[2] == 3:
            lo = mid + 1
        else:
            hi = mid
    return lo


def check_cells(m, start, goal):
    from qtos_amd.global_planner import path_cells
    want = astar_reference(m, start, goal)
    cells, n, status = path_cells(m, start, goal)
    assert cells.dtype == np.int32 and cells.shape == (m.shape[0] * m.shape[1] + 1, 2)
    if want is None:
        assert (n, status) == (0, 1) and not cells.any()
    else:
        assert status == 0 and n == len(want) and [tuple(c) for c in cells[:n]] == want and not cells[n:].any()
    return want


@pytest.mark.parametrize("name", GOLDEN_MAPS)
def test_path_cells_is_astar_on_the_golden_maps(name):
    m = tile_map(name)
    found = [check_cells(m, (0.0, 0.0), goal) is not None for goal in GOLDEN_GOALS]
    assert found == [True, True, True, False]              # (x = 4.7 lies beyond the two tiles: the whole map is searched)


@pytest.mark.parametrize("blocked", [0.10, 0.25, 0.35])
def test_path_cells_is_astar_on_random_grids(blocked):
    rng = np.random.default_rng(int(blocked * 100))
    found = 0
    for _ in range(6):
        m = (rng.random((20, 37)) < blocked) * 1.0         # an odd number of columns
        m[10, 10] = 0.0
        found += check_cells(m, (0.0, 0.0), (2.5, 0.3)) is not None
        found += check_cells(m, (0.05, -0.95), (-0.95, 0.95)) is not None
    assert found >= 1                                      # (at 35 % most goals are walled off: that is status 1, checked above)


def batch_maps():
    m = np.zeros((3, 20, 37))
    m[1, 0:18, 20] = 1.0                                   # a wall with a gap at its top
    m[1, 4:7, 29:32] = 1.0                                 # a box round the cell (5, 30)
    m[1, 5, 30] = 0.0
    rng = np.random.default_rng(39)
    m[2] = (rng.random((20, 37)) < 0.25) * 1.0
    m[2, 10, 10] = 0.0
    return m


# name, map, start (x, y), robot goal (x, y): the batch of the GPU test, one window per case of the issue
BATCH = (("straight", 0, (0.0, 0.0), (1.5, 0.0)), ("detour", 1, (0.0, 0.0), (2.0, 0.0)), ("one cell", 0, (0.01, 0.01), (0.05, 0.06)),
         ("three cells", 0, (0.05, 0.05), (0.25, 0.05)), ("five cells", 0, (0.05, 0.05), (0.45, 0.05)),
         ("start outside", 0, (-1.05, 0.05), (0.5, 0.05)), ("walled in", 1, (0.0, 0.0), (2.05, -0.45)),
         ("too long", 1, (-0.95, -0.95), (2.6, -0.95)), ("open cap", 0, (-0.95, -0.95), (2.65, 0.95)), ("T = 0", 0, (0.3, 0.3), (0.3, 0.3)),
         ("random", 2, (0.0, 0.0), (2.5, 0.3)))
BATCH_STATUS = [0, 0, 0, 0, 0, 0, 1, 2, 3, 4, 0]
BATCH_PARAMS = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=0.5, max_cells=48, max_open=48, max_pieces=24,
                    set_done=True)


def batch_arrays():
    """(maps, map_id, start [B, 24], robot_goal [B, 3], done [B]) of the batch."""
    B = len(BATCH)
    start, goal = np.zeros((B, 24)), np.full((B, 3), 0.24)
    for b, (_, _, s, g) in enumerate(BATCH):
        start[b, 0:3] = [s[0], s[1], 0.24]
        goal[b, 0:2] = g
    start[:, 3:] = np.arange(B * 21).reshape(B, 21)        # (nothing else of a start vector is read)
    done = np.array([0, 1, 0, 2, 0, 0, 0, 1, 0, 2, 0], np.int32)
    return batch_maps(), np.array([c[1] for c in BATCH], np.int32), start, goal, done


@pytest.fixture(scope="module")
def batch_plan():
    from qtos_amd.global_planner import path_plan
    maps, map_id, start, goal, done = batch_arrays()
    return path_plan(maps, map_id, start, goal, BATCH_PARAMS, done=done)


def test_the_batch_holds_the_cases_of_the_issue(batch_plan):
    from qtos_amd.global_planner import path_cells
    maps, map_id, start, goal, done = batch_arrays()
    out = batch_plan
    assert len(BATCH) == 11 and sorted(set(map_id.tolist())) == [0, 1, 2]
    assert out["status"].tolist() == BATCH_STATUS and out["status"].dtype == out["n_cells"].dtype == out["n_pieces"].dtype == np.int32
    assert out["n_cells"].tolist() == [16, 37, 1, 3, 5, 17, 0, 73, 0, 1, 33]
    assert out["n_pieces"].tolist() == [8, 19, 1, 2, 3, 9, 1, 1, 1, 1, 17]
    assert out["cells"][5, 0].tolist() == [10, -1]                             # the start one cell outside the grid
    assert out["cells"][0, :16, 0].tolist() == [10] * 16                       # the straight row
    assert len(set(out["cells"][1, :37, 0].tolist())) > 8                      # the detour leaves its row for the gap
    assert out["done"].tolist() == [0, 1, 0, 2, 0, 0, 4, 5, 4, 6, 0]           # bit 2 where there is no path, the others kept
    assert (done == [0, 1, 0, 2, 0, 0, 0, 1, 0, 2, 0]).all()
    for b, st in enumerate(BATCH_STATUS):
        n = out["n_pieces"][b]
        if st:                                                                 # the constant spine at the start point
            assert n == 1 and not out["knots"][b].any()
            want = np.zeros((2, 4, 24))
            want[:, 3, 0] = start[b, 0:2]
            assert np.array_equal(out["coef"][b], want)
            assert (st in (2, 4)) or not out["cells"][b].any()
        else:
            T = out["knots"][b, n]
            assert T > 0 and (out["knots"][b, n:] == T).all() and (np.diff(out["knots"][b, :n + 1]) > 0).all()
            assert not out["coef"][b, :, :, n:].any() and out["coef"][b, :, 3, 0].tolist() == list(
                out["cells"][b, 0, ::-1] * 0.1 - 1.0)                          # the spine starts in its first cell's corner
    assert same(out["robot_goal"], goal)
    # the two caps sit between what their case needs and what every other case needs
    needs = [open_need(maps[m], s, g) for _, m, s, g in BATCH]
    assert needs[8] > BATCH_PARAMS["max_open"] >= max(needs[:8] + needs[9:])
    lengths = [path_cells(maps[m], s, g)[1] for _, m, s, g in BATCH]
    assert lengths[7] > BATCH_PARAMS["max_cells"] >= max(lengths[:7] + lengths[9:])


def test_status_of_a_walled_in_goal_and_of_the_two_caps():
    from qtos_amd.global_planner import path_cells
    maps = batch_maps()
    s, g = (0.0, 0.0), (2.05, -0.45)
    assert astar_reference(maps[1], s, g) is None
    cells, n, status = path_cells(maps[1], s, g)
    assert (n, status) == (0, 1) and not cells.any()
    # one below what the same case needs
    s, g = (0.0, 0.0), (2.0, 0.0)
    _, n, status = path_cells(maps[1], s, g)
    need = open_need(maps[1], s, g)
    assert (n, status, need) == (37, 0, 41)
    full = path_cells(maps[1], s, g, max_cells=n, max_open=need)
    assert full[1:] == (n, 0) and full[0].shape == (n, 2)
    short = path_cells(maps[1], s, g, max_cells=n - 1, max_open=need)
    assert short[1:] == (n, 2) and not short[0].any()                         # (the length it would have needed is reported)
    assert path_cells(maps[1], s, g, max_cells=n, max_open=need - 1)[1:] == (0, 3)
    # a start or goal whose cell is no number or no int32
    for bad in ((np.nan, 0.0), (0.0, np.inf), (1e12, 0.0), (0.0, -1e300)):
        assert path_cells(maps[0], bad, (1.0, 0.0))[1:] == (0, 1) and path_cells(maps[0], (0.0, 0.0), bad)[1:] == (0, 1)
    # a start far outside the grid is expanded once: none of its neighbours is a cell
    assert path_cells(maps[0], (-7.0, 0.0), (1.0, 0.0))[1:] == (0, 1) and astar_reference(maps[0], (-7.0, 0.0), (1.0, 0.0)) is None
    # a grid of one row
    assert path_cells(np.zeros((1, 3)), (-0.95, -0.95), (-0.75, -0.95))[1:] == (3, 0)


def knots_of(n, T):
    t = np.arange(n + 1) * (T / n)
    t[n] = T
    return t


def step_path(n, rng):
    """Points as a path gives them: steps of 0 or 0.2, and the last point without the origin shift."""
    y = np.cumsum(rng.integers(0, 2, n + 1)) * 0.2 - 1.0
    y[-1] += 1.0
    return y


def test_spine_fit_is_cubic_spline_within_the_gate():
    from qtos_amd.global_planner import spine_fit
    worst = {}
    for n in [1, 2, 3] + list(range(4, 40)) + [80, 141]:
        for seed in range(20):
            rng = np.random.default_rng(1000 * n + seed)
            t, y = knots_of(n, rng.uniform(1.0, 400.0)), step_path(n, rng)
            c, w = spine_fit(t, y), CubicSpline(t, y).c
            assert c.shape == w.shape == (4, n)
            worst[n] = max(worst.get(n, 0.0), fit_error(c, w))
    print("spine_fit against scipy: worst %.3g (n = 1: %.3g, n = 2: %.3g, n = 3: %.3g); measured %.3g, gate %.3g" % (
        max(worst.values()), worst[1], worst[2], worst[3], FIT_MEASURED, FIT_GATE))
    assert max(worst.values()) <= FIT_GATE, worst
    # the line and the parabola are what they are called
    c = spine_fit([0.0, 4.0], [1.0, 3.0])
    assert c.tolist() == [[0.0], [0.0], [0.5], [1.0]]
    c = spine_fit([0.0, 1.0, 3.0], [0.0, 1.0, 9.0])        # y = t^2
    assert np.allclose(c, [[0.0, 0.0], [1.0, 1.0], [0.0, 2.0], [0.0, 1.0]], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        spine_fit([0.0], [1.0])


def golden_planner(name, goal, step_size=1.0):
    from qtos_amd.global_planner import GlobalPlanner
    gp = GlobalPlanner(tile_map(name), [0.0, 0.0, 0.24], [goal[0], goal[1], 0.24], step_size=step_size, resolution=0.1)
    assert gp.path_solver.solution_flag
    return gp


def test_path_plan_is_path_table_of_the_global_planner():
    from qtos_amd.global_planner import path_goal, path_plan, path_table
    cases = [(name, goal) for name in GOLDEN_MAPS for goal in GOLDEN_GOALS[:3]]
    gps = [golden_planner(name, goal) for name, goal in cases]
    want = path_table(gps)
    B = len(cases)
    maps = np.stack([tile_map(name) for name in GOLDEN_MAPS])
    map_id = np.array([GOLDEN_MAPS.index(name) for name, _ in cases])
    start = np.zeros((B, 24))
    start[:, 2] = 0.24
    goal = np.array([[g[0], g[1], 0.24] for _, g in cases])
    mp = want["coef"].shape[3]
    par = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=1.0, max_cells=2 * mp, max_open=4096, max_pieces=mp,
               set_done=False)
    got = path_plan(maps, map_id, start, goal, par)
    assert not got["status"].any() and "done" not in got
    assert np.array_equal(got["n_pieces"], want["n_pieces"]) and got["knots"].shape == want["knots"].shape
    assert same(got["robot_goal"], want["robot_goal"])
    for b, gp in enumerate(gps):
        assert [tuple(c) for c in got["cells"][b, :got["n_cells"][b]]] == gp.path_solver.path
    # knots: np.linalg.norm may fuse its dot product, the rest of the chain is the same operations: 4 ulp
    ulp = np.abs(bits(got["knots"]) - bits(want["knots"])).max()
    print("knots: %d ulp" % ulp)
    assert ulp <= 4
    worst = max(fit_error(got["coef"][b, a, :, :n], want["coef"][b, a, :, :n]) for b, n in enumerate(want["n_pieces"]) for a in (0, 1))
    print("coef against scipy on the golden paths: %.3g (gate %.3g)" % (worst, FIT_GATE))
    assert worst <= FIT_GATE
    for b, n in enumerate(want["n_pieces"]):
        assert not got["coef"][b, :, :, n:].any() and (got["knots"][b, n:] == got["knots"][b, n]).all()
    # the goals of five replans from both tables
    grids, clock = maps[map_id], np.zeros(B)
    state = start.copy()
    for k in range(5):
        off = np.full(B, 2.5 + 0.1 * k)
        a = path_goal(got, None, grids, np.arange(B), clock, off, state, dict(REF, base="state", step_size=0.6))
        w = path_goal(want, None, grids, np.arange(B), clock, off, state, dict(REF, base="state", step_size=0.6))
        diff = np.abs(a[0] - w[0]).max()
        assert diff <= FIT_GATE * (k + 1) * max(1.0, np.abs(w[0]).max()), (k, diff)
        assert np.array_equal(a[1], w[1])
        clock, state[:, 0:3] = w[2], w[0]


def test_params_struct_mirrors_the_dict(batch_plan):
    from qtos_amd import capi
    from qtos_amd.global_planner import path_plan
    maps, map_id, start, goal, done = batch_arrays()
    g = capi.path_plan_params(step_size=0.5, max_cells=48, max_open=48, max_pieces=24, set_done=True, bool_map=maps)
    assert (g.n_maps, g.rows, g.cols, g.cell, g.origin_x, g.origin_y, g.height_bound) == (3, 20, 37, 0.1, 1.0, 1.0, 0.2)
    out = path_plan(maps, map_id, start, goal, g, done=done)
    for key, v in batch_plan.items():
        assert same(out[key], v) if v.dtype == np.float64 else np.array_equal(out[key], v), key
    d = capi.path_plan_params(bool_map=maps[0])
    assert (d.n_maps, d.max_cells, d.max_pieces, d.max_open, d.set_done) == (1, 114, 57, 4096, 0)
    for bad in (dict(max_open=4097), dict(max_cells=49), dict(max_open=0)):
        with pytest.raises(ValueError):
            path_plan(maps, map_id, start, goal, dict(BATCH_PARAMS, **bad))
    with pytest.raises(ValueError):
        path_plan(np.zeros((1, 129, 128)), None, start, goal, BATCH_PARAMS)


FIELDS = ("rows", "cols", "cell", "origin_x", "origin_y", "height_bound", "step_size", "max_cells", "max_open", "max_pieces", "n_maps",
          "set_done")


def test_abi_exports_and_struct_size(tmp_path):
    from qtos_amd import capi
    from qtos_amd.global_planner import PATH_PLAN_FIELDS
    lib = capi.load()
    assert "qtos_path_plan" in capi.EXPORTS and "qtos_path_plan_device" in capi.EXPORTS
    assert hasattr(lib, "qtos_path_plan") and hasattr(lib, "qtos_path_plan_device")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qtos_planner.h"\n'
                   'typedef int (*host_form)(QtosPlanner *, int, const QtosPathPlan *, const double *, const int *, const double *, const double *,\n'
                   '                         double *, double *, int *, int *, int *, int *, int *);\n'
                   'typedef int (*device_form)(QtosPlanner *, int, const QtosPathPlan *, const double *, const int *, const double *, const double *,\n'
                   '                           double *, double *, int *, int *, int *, int *, int *, void *);\n'
                   'int main(void) {\n  host_form h = &qtos_path_plan;\n  device_form d = &qtos_path_plan_device;\n'
                   '  printf("%d %d", (int)sizeof(QtosPathPlan), h != NULL && d != NULL);\n'
                   + "".join('  printf(" %%d", (int)offsetof(QtosPathPlan, %s));\n' % f for f in FIELDS) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-lqtos_planner", "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.QtosPathPlan
    assert [name for name, _ in S._fields_] == list(FIELDS) == list(PATH_PLAN_FIELDS)
    assert got == [C.sizeof(S), 1] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 72
    # the argument check that needs no planner
    buf, ints = np.zeros(2000), np.zeros(200, np.int32)
    ok = capi.path_plan_params(bool_map=np.zeros((4, 4)))
    assert lib.qtos_path_plan(None, 1, C.byref(ok), capi._dp(buf), None, capi._dp(buf), capi._dp(buf), capi._dp(buf), capi._dp(buf),
                              capi._ip(ints), capi._ip(ints), capi._ip(ints), capi._ip(ints), None) == -1
    assert lib.qtos_path_plan_device(None, 1, C.byref(ok), *([None] * 12)) == -1


def test_c99_caller_builds_and_checks_its_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "pathplan_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "pathplan_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_path_plan"]) == C.sizeof(capi.QtosPathPlan)
    assert int(kv["path_plan_null"]) == -1 and int(kv["path_plan_device_null"]) == -1


def test_k_path_plan_uses_no_scratch_and_the_documented_lds(notes):  # noqa: F811
    block = one_kernel(notes, "k_path_plan")
    assert field(block, "private_segment_fixed_size") == 0, "scratch bytes per lane (ScratchSize)"
    assert 0 < field(block, "group_segment_fixed_size") <= LDS_BYTES, "LDS bytes"
    assert field(block, "vgpr_spill_count") == 0 and field(block, "sgpr_spill_count") == 0
    assert field(block, "max_flat_workgroup_size") == 64
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "%d B" % LDS_BYTES in design and "Path-plan kernel" in design
