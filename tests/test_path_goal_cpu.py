"""Goals of receding windows from their global paths without a GPU: the numpy statement of k_path_goal's rule
(global_planner.spine_eval, map_height, path_table, path_goal) against scipy's CubicSpline and the GlobalPlanner, which is pinned to
the reference, to the bit; the C ABI of qtos_path_goal*, the C99 loop's build and argument checks, and the resources of
k_path_goal read from the gfx950 code object."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
from scipy.interpolate import CubicSpline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_stitch_cpu import CSRC, field, notes, one_kernel  # noqa: E402,F401  (the code object's notes, read as that file reads them)

GOLDEN = os.path.join(ROOT, "tests", "golden")
PIECES = (1, 2, 3, 11)
REF = dict(horizon=5.0, step_size=1.0, tol=1e-5, z_offset=0.24, cell=0.1, origin_x=1.0, origin_y=1.0, t_stop=7.5, stop_dist=0.0,
           base="spine", clamp_x=False, advance_clock=True, hold_done=False)     # the reference's constants


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def same(a, b):
    """Equal to the bit; a NaN equals a NaN (IEEE leaves its payload open)."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


class Spine:
    """What path_table reads of a PathSolver."""

    def __init__(self, n, rng, robot_goal=None):
        t = np.concatenate([[0.0], np.cumsum(rng.uniform(0.3, 2.0, n))])
        self.spine_x_track = CubicSpline(t, rng.standard_normal(n + 1))
        self.spine_y_track = CubicSpline(t, rng.standard_normal(n + 1))
        if robot_goal is not None:
            self.robot_goal = robot_goal


def queries(x, rng):
    """Before the first knot, every knot exactly (the last included), beyond the end, and random interior times."""
    return np.concatenate([[x[0] - 3.7, x[0] - 1e-9, np.nextafter(x[0], -np.inf)], x, np.nextafter(x[1:], -np.inf), np.nextafter(x[:-1], np.inf),
                           [x[-1] + 1e-9, x[-1] + 12.3, x[-1] + 1e6], rng.uniform(x[0], x[-1], 200)])


@pytest.mark.parametrize("n", PIECES)
def test_spine_eval_is_cubic_spline_call_to_the_bit(n):
    from qtos_amd.global_planner import path_table, spine_eval
    rng = np.random.default_rng(100 + n)
    for _ in range(5):
        sp = Spine(n, rng)
        tab = path_table([sp])
        assert tab["n_pieces"].tolist() == [n] and tab["knots"].shape == (1, n + 1) and tab["coef"].shape == (1, 2, 4, n)
        for axis, cs in enumerate((sp.spine_x_track, sp.spine_y_track)):
            assert cs.c.shape == (4, n)
            for t in queries(cs.x, rng):
                got, want = spine_eval(tab["knots"][0], tab["coef"][0, axis], n, t), cs(t)
                assert bits(got) == bits(want), (n, axis, t, float(got), float(want))
    # a NaN time is a NaN, as scipy gives it
    assert np.isnan(spine_eval(tab["knots"][0], tab["coef"][0, 0], n, np.nan)) and np.isnan(sp.spine_x_track(np.nan))


def test_path_table_pads_and_a_padded_row_evaluates_like_the_spline():
    from qtos_amd.global_planner import _spine_eval_rows, path_table, spine_eval
    rng = np.random.default_rng(7)
    spines = [Spine(n, rng, robot_goal=[1.0 + n, 0.5]) for n in PIECES]
    spines[1] = Spine(2, rng)                                           # (one without a robot goal)
    tab = path_table(spines)
    assert tab["knots"].shape == (4, 12) and tab["coef"].shape == (4, 2, 4, 11) and tab["robot_goal"].shape == (4, 3)
    assert tab["n_pieces"].dtype == np.int32 and tab["n_pieces"].tolist() == list(PIECES)
    assert tab["robot_goal"][0].tolist()[:2] == [2.0, 0.5] and np.isnan(tab["robot_goal"][0, 2]) and np.isnan(tab["robot_goal"][1]).all()
    for j, (sp, n) in enumerate(zip(spines, PIECES)):
        x = sp.spine_x_track.x
        assert np.array_equal(tab["knots"][j, :n + 1], x) and (tab["knots"][j, n + 1:] == x[-1]).all()
        assert np.array_equal(tab["coef"][j, 0, :, :n], sp.spine_x_track.c) and np.array_equal(tab["coef"][j, 1, :, :n], sp.spine_y_track.c)
        assert (tab["coef"][j, :, :, n:] == 0).all()
        ts = queries(x, rng)
        for axis, cs in enumerate((sp.spine_x_track, sp.spine_y_track)):
            want = cs(ts)
            got = np.array([spine_eval(tab["knots"][j], tab["coef"][j, axis], n, t) for t in ts])
            assert same(got, want), (j, axis)
            # and the batched form path_goal uses
            m = len(ts)
            rows = _spine_eval_rows(np.repeat(tab["knots"][j][None], m, 0), np.repeat(tab["coef"][j, axis][None], m, 0), np.full(m, n), ts)
            assert same(rows, want), (j, axis)
    with pytest.raises(ValueError):
        path_table([])


def tile_map(name):
    from qtos_amd import heightfield
    tiles = [heightfield.read_tile(os.path.join(GOLDEN, "heightfields", t + ".txt")) for t in (name, "plane")]
    return heightfield.build_map(tiles, 1)


def test_map_height_is_get_map_height():
    from qtos_amd.global_planner import GlobalPlanner, map_height
    rng = np.random.default_rng(11)
    m = tile_map("climb_1") + 0.001 * rng.standard_normal((20, 40))     # (every cell its own value)
    gp = GlobalPlanner(np.zeros((20, 40)), [0, 0, 0.24], [1.5, 0, 0.24])
    gp.map = m
    pts = [(x, y) for x in rng.uniform(-1.0, 3.0, 12) for y in rng.uniform(-1.0, 1.0, 5)]           # interior cells
    pts += [(-1.05, 0.0), (-2.3, 0.4), (0.5, -1.01), (0.5, -2.95), (-4.99, -2.99), (-5.0, -3.0)]    # left / below the origin: wrap
    pts += [(-5.01, 0.0), (0.0, -3.01), (-9.0, -9.0), (3.0, 0.0), (3.7, 0.0), (0.0, 1.0), (0.0, 5.5), (1e300, 0.0), (0.0, -1e300)]  # fall back
    pts += [(np.nan, 0.0), (0.0, np.nan), (np.nan, np.nan), (np.inf, 0.0), (0.0, -np.inf)]
    pts += [(-1.0, -1.0), (2.9999999, 0.9999999), (0.0, 0.0)]
    want = np.array([gp.get_map_height(p) for p in pts])
    got = map_height(m, [p[0] for p in pts], [p[1] for p in pts], 0.1, 1.0, 1.0)
    assert np.array_equal(bits(got), bits(want)), np.argwhere(bits(got) != bits(want))
    fallback = m[19, 20]
    assert got[60 + 6] == fallback and got[60 + 6 + 8] == fallback and (got[60 + 15:60 + 20] == fallback).all()
    assert got[60] == m[10, 39] != fallback                             # (-1.05, 0.0): row 10, col -1
    # one grid per point
    many = map_height(np.stack([m, 2.0 * m]), [0.3, 0.3], [0.1, 0.1], 0.1, 1.0, 1.0)
    assert many[0] == m[11, 13] and many[1] == 2.0 * m[11, 13]


def planners(step_size):
    from qtos_amd.global_planner import GlobalPlanner
    out = []
    for name, goal in (("climb_1", [2.5, 0.0, 0.24]), ("plane", [0.8, 0.3, 0.24])):
        gp = GlobalPlanner(tile_map(name), [0, 0, 0.24], goal, step_size=step_size, resolution=0.1, lookahead=0)
        assert gp.path_solver.solution_flag and gp.lookahead_timestamp(1.37) == 1.37      # (lt is exactly the time passed)
        out.append(gp)
    return out


def times(gp):
    return 0.37 * np.arange(int((gp.max_t + 10.0) / 0.37) + 1)


@pytest.mark.parametrize("step_size", [1.0, 0.25])
def test_base_spine_is_global_planner_update(step_size):
    from qtos_amd.global_planner import path_goal, path_table
    gps = planners(step_size)
    tab = path_table(gps)
    assert np.array_equal(tab["robot_goal"], [[2.5, 0.0, 0.24], [0.8, 0.3, 0.24]])
    maps = np.stack([gp.map for gp in gps])
    for j, gp in enumerate(gps):
        ts = times(gp)
        assert ts[0] == 0 and ts[-1] > gp.max_t + 9.6
        want_start, want_goal = [], []
        for t in ts:
            gp.update(t)
            s, g = gp.pop()
            want_start.append(s), want_goal.append(g)
        B = len(ts)
        goal, done, clock = path_goal(tab, np.full(B, j), maps, np.full(B, j), ts, None, None, dict(REF, step_size=step_size))
        assert same(goal, want_goal), (j, np.argwhere(bits(goal) != bits(np.array(want_goal)))[:5])
        assert np.array_equal(bits(clock), bits(ts))
        assert done.dtype == np.int32 and np.array_equal(done != 0, gp.max_t < ts - 7.5) and done.any() and not done.all()
        # the pair's start is the rule's base point: a step of size 0 stays on it
        base, _, _ = path_goal(tab, np.full(B, j), maps, np.full(B, j), ts, None, None, dict(REF, step_size=0.0))
        assert np.array_equal(base, want_start)
        # and the goal is the clipped step from that start
        state = np.zeros((B, 24))
        state[:, 0:3] = want_start
        goal2, _, _ = path_goal(tab, np.full(B, j), maps, np.full(B, j), ts, None, state, dict(REF, step_size=step_size, base="state"))
        assert same(goal2, want_goal)
    if step_size < 1.0:
        moved = np.abs(np.array(want_goal) - np.array(want_start)).max(axis=0)[:2]
        assert (np.abs(moved - step_size) < 1e-12).all()                # (the clip was met)


def test_base_state_is_spine_step():
    from qtos_amd.global_planner import path_goal, path_table
    rng = np.random.default_rng(5)
    gps = planners(0.25)
    tab = path_table(gps)
    maps = np.stack([gp.map for gp in gps])
    for j, gp in enumerate(gps):
        ts = times(gp)
        B = len(ts)
        state = np.zeros((B, 24))
        state[:, 0:3] = rng.uniform([-0.5, -0.5, 0.2], [2.5, 0.5, 0.3], (B, 3))
        off = rng.uniform(0.0, 3.0, B)
        goal, _, clock = path_goal(tab, np.full(B, j), maps, np.full(B, j), ts - off, off, state,
                                   dict(REF, step_size=0.25, base="state", advance_clock=False))
        lt = (ts - off) + off
        want = np.array([gp.spine_step(state[k, 0:3], lt[k]) for k in range(B)])
        assert same(goal, want)
        assert np.array_equal(bits(clock), bits(ts - off))              # (the clock stays without advance_clock)


def test_clamp_x_is_combiner_spine_step():
    from qtos_amd.global_planner import path_goal, path_table
    rng = np.random.default_rng(9)
    gp = planners(0.3)[0]
    gp.robot_goal = [1.2, 0.0, 0.24]                                    # (the path runs on to x = 2.5: the clamp is met)
    tab = path_table([gp])
    ts = times(gp)
    B = len(ts)
    state = np.zeros((B, 24))
    state[:, 0:3] = rng.uniform([0.0, -0.3, 0.2], [2.0, 0.3, 0.3], (B, 3))
    sx, sy = gp.path_solver.spine_x_track, gp.path_solver.spine_y_track

    def combiner_spine_step(com, timestep, total_traj_time=5.0):        # QTOS/combiner.py:194-212, written out
        tf = timestep + total_traj_time
        z_goal = gp.get_map_height((sx(tf), sy(tf)))
        goal = np.array([sx(tf), sy(tf), z_goal + 0.24])
        if goal[0] > gp.robot_goal[0]:
            goal[0] = gp.robot_goal[0]
        return com + np.clip(goal - com, -0.3, 0.3)

    want = np.array([combiner_spine_step(state[k, 0:3], ts[k]) for k in range(B)])
    par = dict(REF, step_size=0.3, base="state", clamp_x=True, tol=0.0)  # (Combiner.spine_step has no tol rule)
    goal, _, _ = path_goal(tab, np.zeros(B, np.int64), gp.map, None, ts, None, state, par)
    assert same(goal, want)
    clamped = np.array([sx(t + 5.0) > 1.2 for t in ts])
    assert clamped.any() and not clamped.all()
    free, _, _ = path_goal(tab, np.zeros(B, np.int64), gp.map, None, ts, None, state, dict(par, clamp_x=False))
    differ = bits(free) != bits(goal)
    assert not differ[~clamped].any() and not differ[:, 1:].any() and differ[clamped, 0].any()     # (the clamp moves x alone)


def two_piece_table():
    """x(t) = 0.08 t and a C2 cubic in y over the knots 0, 10, 20 (the path of tests/c/path_caller.c)."""
    coef = np.zeros((1, 2, 4, 2))
    coef[0, 0, 2], coef[0, 0, 3] = [0.08, 0.08], [0.0, 0.8]
    coef[0, 1] = [[2e-5, -2e-5], [0.0, 0.0006], [0.0, 0.006], [0.0, 0.02]]
    return dict(knots=np.array([[0.0, 10.0, 20.0]]), coef=coef, n_pieces=np.array([2], np.int32), robot_goal=np.array([[1.6, 0.12, 0.24]]))


def test_done_bits_are_sticky_and_hold_and_clock():
    from qtos_amd.global_planner import path_goal
    tab = two_piece_table()
    pid = np.zeros(6, np.int64)
    clock = np.array([0.0, 27.0, 27.6, 3.0, 3.0, 30.0])
    offset = np.array([2.5, 0.5, 0.0, 2.5, 2.5, 2.5])
    start = np.zeros((6, 24))
    start[:, 0] = [0.1, 1.9, 1.9, 0.84, 0.5, 2.0]
    start[:, 1] = [0.0, 0.1, 0.1, 0.04, 0.0, 0.1]
    start[:, 2] = 0.24
    done_in = np.array([0, 0, 0, 0, 4, 0], np.int32)
    par = dict(REF, step_size=0.45, stop_dist=0.05, t_stop=7.5, base="spine", hold_done=False)
    goal, done, clock_out = path_goal(tab, pid, None, None, clock, offset, start, par, done=done_in)
    # bit 0: t_end = 20 < lt - 7.5, strictly: lt = 27.5 is not yet done, 27.6 is
    # bit 1: window 3 starts within 0.05 of its goal -- lt = 5.5, tf = 10.5, the spine moves 0.4 < step_size: the goal is X(10.5), Y(10.5)
    assert np.allclose(goal[3], [0.84, 0.02 + 0.003 + 0.00015 - 2.5e-6, 0.24], rtol=0, atol=1e-15)
    assert done.tolist() == [0, 0, 1, 2, 4, 1] and done.dtype == np.int32
    assert np.array_equal(clock_out, clock + offset) and (goal[:, 2] == 0.24).all()       # (no grid: every height 0)
    assert (done_in == [0, 0, 0, 0, 4, 0]).all()                        # (new arrays)
    # sticky: the bits a window has stay whatever the new ones are, and hold_done puts a done window's goal on its start
    held, done2, _ = path_goal(tab, pid, None, None, clock, offset, start, dict(par, hold_done=True), done=done)
    assert done2.tolist() == [0, 0, 1, 2, 4, 1]
    assert np.array_equal(bits(held[2:]), bits(start[2:, 0:3])) and np.array_equal(bits(held[:2]), bits(goal[:2]))
    # without the clock
    _, _, kept = path_goal(tab, pid, None, None, clock, offset, start, dict(par, advance_clock=False), done=done_in)
    assert np.array_equal(kept, clock) and kept is not clock
    # stop_dist 0: no bit 1; done None: the bits of this call alone
    _, done3, _ = path_goal(tab, pid, None, None, clock, offset, start, dict(par, stop_dist=0.0))
    assert done3.tolist() == [0, 0, 1, 0, 0, 1]
    # start is needed where it is read
    for bad in (dict(par), dict(par, stop_dist=0.0, hold_done=True), dict(par, stop_dist=0.0, base="state")):
        with pytest.raises(ValueError):
            path_goal(tab, pid, None, None, clock, offset, None, bad)
    path_goal(tab, pid, None, None, clock, offset, None, dict(par, stop_dist=0.0))
    # a NaN clock: the spine is NaN, the clip keeps it, and no bit is set; the tol rule and the height rule read a NaN as the
    # reference does (0.0, the fall-back cell), so the goal's height stays a number with base "spine"
    g, d, c = path_goal(tab, pid[:1], None, None, [np.nan], None, None, dict(par, stop_dist=0.0))
    assert np.isnan(g[0, 0]) and np.isnan(g[0, 1]) and g[0, 2] == 0.24 and d.tolist() == [0] and np.isnan(c[0])


def test_params_struct_mirrors_the_dict():
    from qtos_amd import capi
    from qtos_amd.global_planner import path_goal
    tab = two_piece_table()
    grid = np.arange(800.0).reshape(20, 40) * 1e-3
    g = capi.path_goal_params(5.0, 0.45, 1e-5, 0.24, 0.1, (1.0, 1.0), 7.5, 0.05, "state", True, False, True, table=tab, map_yx=grid)
    assert (g.n_paths, g.max_pieces, g.n_maps, g.rows, g.cols) == (1, 2, 1, 20, 40)
    assert (g.base, g.clamp_x, g.advance_clock, g.hold_done) == (1, 1, 0, 1)
    d = dict(REF, step_size=0.45, stop_dist=0.05, base="state", clamp_x=True, advance_clock=False, hold_done=True)
    clock = np.array([0.0, 9.0, 28.0])
    start = np.zeros((3, 24))
    start[:, 0:3] = [[0.0, 0.0, 0.24], [1.0, 0.0, 0.25], [2.0, 0.1, 0.24]]
    a = path_goal(tab, np.zeros(3, np.int32), grid, None, clock, None, start, g)
    b = path_goal(tab, np.zeros(3, np.int32), grid, None, clock, None, start, d)
    assert all(same(u, v) for u, v in zip(a, b))
    assert capi.path_goal_params().base == 0 and capi.path_goal_params(map_yx=np.zeros((3, 20, 40))).n_maps == 3


FIELDS = ("horizon", "step_size", "tol", "z_offset", "cell", "origin_x", "origin_y", "t_stop", "stop_dist", "base", "clamp_x",
          "advance_clock", "hold_done", "n_paths", "max_pieces", "n_maps", "rows", "cols")


def test_abi_exports_and_struct_size(tmp_path):
    from qtos_amd import capi
    lib = capi.load()
    assert "qtos_path_goal" in capi.EXPORTS and "qtos_path_goal_device" in capi.EXPORTS
    assert hasattr(lib, "qtos_path_goal") and hasattr(lib, "qtos_path_goal_device")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qtos_planner.h"\n'
                   'typedef int (*host_form)(QtosPlanner *, int, const QtosPathGoal *, const double *, const double *, const int *, const double *,\n'
                   '                         const int *, const double *, const int *, double *, const double *, const double *, double *, int *);\n'
                   'typedef int (*device_form)(QtosPlanner *, int, const QtosPathGoal *, const double *, const double *, const int *, const double *,\n'
                   '                           const int *, const double *, const int *, double *, const double *, const double *, double *, int *, void *);\n'
                   'int main(void) {\n  host_form h = &qtos_path_goal;\n  device_form d = &qtos_path_goal_device;\n'
                   '  printf("%d %d", (int)sizeof(QtosPathGoal), h != NULL && d != NULL);\n'
                   + "".join('  printf(" %%d", (int)offsetof(QtosPathGoal, %s));\n' % f for f in FIELDS) +
                   '  printf("\\n");\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", CSRC, "-lqtos_planner", "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.QtosPathGoal
    assert [name for name, _ in S._fields_] == list(FIELDS)
    assert got == [C.sizeof(S), 1] + [getattr(S, f).offset for f in FIELDS]
    assert C.sizeof(S) == 112
    # the argument checks that need no planner
    buf = np.zeros(24)
    ok = capi.path_goal_params(table=two_piece_table())
    one = np.ones(1, np.int32)
    assert lib.qtos_path_goal(None, 1, C.byref(ok), capi._dp(buf), capi._dp(buf), capi._ip(one), None, None, None, None, capi._dp(buf), None,
                              None, capi._dp(buf), None) == -1
    assert lib.qtos_path_goal_device(None, 1, C.byref(ok), *([None] * 13)) == -1


def test_c99_path_loop_builds_and_checks_its_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "path_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "path_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_path_goal"]) == C.sizeof(capi.QtosPathGoal)
    assert int(kv["path_goal_null"]) == -1 and int(kv["path_goal_device_null"]) == -1


def test_k_path_goal_uses_no_scratch_and_no_lds(notes):  # noqa: F811
    block = one_kernel(notes, "k_path_goal")
    assert field(block, "private_segment_fixed_size") == 0, "scratch bytes per lane (ScratchSize)"
    assert field(block, "group_segment_fixed_size") == 0, "LDS bytes"
    assert field(block, "vgpr_spill_count") == 0 and field(block, "sgpr_spill_count") == 0
    assert field(block, "max_flat_workgroup_size") == 64
