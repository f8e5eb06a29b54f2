"""The terrain look-up of the kernels (terrain_at in csrc/kernels.hpp) against its index-free statement (oracle/terrain.py) at the
places where the rule decides: on nodes, grid lines and borders, beyond the borders, far beyond them (grid coordinates beyond
int and int64), on nearest-cell ties, on maps with a single row or column, with map ids outside the stack.  pytest -m gpu.

One planner of the smallest transcription (linearisation_cases "two_base_polys", every row of the NLP in the KKT system,
max_batch 32) per terrain mode serves every test.

  (a) eval_all through debug_eval (what k_start and k_step linearise): the free feet of as many evaluation points as the table
      needs stand on the probes of terrain_cases.table -- every probe under a terrain row and under a stance foothold's force
      rows, asserted from the layout.  Terrain rows z - h and their entries -hx, -hy, 1 with == on the dyadic grids (every
      intermediate is exact there: terrain_cases.py), force rows and their entries (the only place hxy shows) within the gate
      of oracle.terrain.force_rows.  Five grid shapes, a stack of three maps with map ids -1 and n_maps among them (clamped
      to the first and last map), and the product's exp_5 grid under the measured gate.
  (b) k_plan_check as a sampler of the look-up: three windows whose feet sweep from beyond the first border to beyond the last
      (terrain_cases.sweep_plans), columns 19 .. 22 against foot z minus the statement's h at the positions Planner.sample
      returns for the same rows, columns 23 .. 26 through force_rows.  Left out of 19 .. 22: where h itself jumps within 1e-9
      cells -- the nearest-cell ties; the bilinear h is continuous, so nothing is, and the stances that stand exactly on a
      node or a border are compared.  Left out of 23 .. 26 as well: rows at a phase switch (the existing decided mask) and, in
      bilinear mode, feet within 1e-9 cells of a line, where the slopes jump.  The ramp reaches the classes up to two cells
      beyond a border; a row exactly on a tie would be left out in nearest-cell mode, so ties are crossed by swings only; the
      classes from 10^6 cells on are in (a) and (c).
  (c) the consumers that read the height only: the starting point (k_debug_guess) and k_shift_warm against Oracle.initial_guess
      with goals beyond a border, exactly on the last border line and far (3 10^9, 10^12 cells); k_start_feedback with the
      corrected feet at such places, its snapped z against the statement with == and the rest against feedback.start_feedback
      with terrain_lookup; k_force_fit on the sweep plan of (b) against force_fit.py with its own gates (the plan is random,
      its feet far apart: the fit's condition number of 10^7 makes those gates wide, and in bilinear mode only the rows
      without a stance foot on a line, 93 of 1800, are decided).  test_terrain_cpu.py ties those restatements to the
      statement.

Every test prints its figures (terrain_cases.record) before it asserts; profiles/terrain_accuracy.json is an MI355X run."""
import dataclasses

import numpy as np
import pytest

import force_fit_cases as ffc
import linearisation_cases as lc
import plan_check_cases as pcc
import spline_cases as sc
import terrain_cases as tc
from oracle import terrain as ot

pytestmark = pytest.mark.gpu
LD, F64 = np.longdouble, np.float64
MODE_NAME = {0: "bilinear", 1: "nearest"}
DYADIC = (tc.CELL, tc.X0, tc.Y0)
LINE_TOL = 1e-12                                          # test_gpu_splines.py: variables that come from the straight line


@pytest.fixture(scope="module", params=[0, 1], ids=["bilinear", "nearest"])
def planner(request):
    from qtos_amd.capi import Planner
    mode = request.param
    cfg = dataclasses.replace(lc.full(lc.case(tc.CASE)[0]), terrain_mode=mode)
    P = Planner(cfg, max_batch=tc.MAX_BATCH)
    yield mode, cfg, P
    P.close()


# ---- (a) eval_all ------------------------------------------------------------------------------------------------------------

def _eval(P, mode, probes, maps, grid, map_id=None, exact=True):
    """debug_eval with the feet on the probes against the statement; returns the record's entry."""
    cell, x0, y0 = grid
    maps = np.asarray(maps, F64)
    x, start, goal, at = tc.eval_points(probes)
    B = len(x)
    mid = None if map_id is None else np.resize(np.array(map_id, np.int32), B)
    terr, force = tc.coverage(probes, at)
    assert terr == force == set(probes.names)             # every probe under a terrain row and under a force instance

    def H_of(b, shift=0):
        m = 0 if mid is None else (min(max(int(mid[b]), 0), len(maps) - 1) + shift) % len(maps)
        return maps[m], cell, x0, y0
    P.set_heightfields(maps, cell, x0, y0)
    g, J = P.debug_eval(start, goal, x, map_id=mid)
    rk, vf, _ = P.structure()
    fx = lc.fixed(tc.CASE)
    assert np.array_equal(vf == 0, fx)
    E, F = (tc.masked(tc.expected(x, H_of, mode, dt), fx, rk) for dt in (LD, F64))
    on = at[:, E["terrain_var"]] >= 0
    entry = dict(problems=B, probes=len(probes), terrain_rows_on_probes=int(on.sum()), floor={}, gate={}, achieved={})
    for k, rows in (("terrain", E["terrain_rows"]), ("force", E["force_rows"])):
        for what, kind, got in (("values", "value", g[:, rows]), ("entries", "entry", J[:, rows])):
            ref, f64 = E[k + ("_g" if what == "values" else "_J")], F[k + ("_g" if what == "values" else "_J")]
            key = k + "_" + what
            entry["floor"][key] = tc.dist(f64, ref)
            entry["gate"][key] = tc.gate(kind, entry["floor"][key])
            entry["achieved"][key] = tc.dist(got, ref)
    if exact:
        tg, tJ = g[:, E["terrain_rows"]], J[:, E["terrain_rows"]]
        assert tc.dist(F["terrain_g"][on], E["terrain_g"][on]) == 0 and tc.dist(F["terrain_J"][on], E["terrain_J"][on]) == 0
        entry["terrain_values_unequal"] = int((tg[on] != F["terrain_g"][on]).sum())
        entry["terrain_entries_unequal"] = int((tJ[on] != F["terrain_J"][on]).sum())
        bad = np.nonzero((tg != F["terrain_g"]) & on)
        entry["first_unequal"] = probes.names[at[bad[0][0], E["terrain_var"][bad[1][0]]]] if len(bad[0]) else None
    if mid is not None:                                   # the maps are told apart: another map's rows are far off
        other = tc.expected(x, lambda b: H_of(b, 1), mode, F64)
        entry["distance_from_another_maps_rows"] = tc.dist(g[:, E["terrain_rows"]][on], other["terrain_g"][on])
    return entry


def _assert_eval(entry, exact=True):
    for k, v in entry["achieved"].items():
        assert v <= entry["gate"][k], (k, v, entry["gate"][k])
    if exact:
        assert entry["terrain_values_unequal"] == 0 and entry["terrain_entries_unequal"] == 0, entry


@pytest.mark.parametrize("shape", list(tc.SHAPES))
def test_eval_all_on_the_dyadic_table(planner, shape):
    mode, cfg, P = planner
    entry = _eval(P, mode, tc.table(tc.SHAPES[shape]), tc.grid(shape)[None], DYADIC)
    tc.record("gpu_eval_" + MODE_NAME[mode], shape, entry)
    _assert_eval(entry)
    if mode == 0 and shape == "5x7":
        assert entry["floor"]["force_entries"] > 0        # hxy does enter


def test_eval_all_on_a_stack_of_maps_with_ids_outside_it(planner):
    mode, cfg, P = planner
    assert {-1, 3} < set(tc.STACK_MAP_ID) and len(tc.stack()) == 3
    entry = _eval(P, mode, tc.table(tc.STACK_SHAPE), tc.stack(), DYADIC, map_id=tc.STACK_MAP_ID)
    tc.record("gpu_eval_" + MODE_NAME[mode], "stack", entry)
    _assert_eval(entry)
    assert entry["distance_from_another_maps_rows"] > 2.0 ** -10


def test_eval_all_on_the_product_grid(planner):
    mode, cfg, P = planner
    H, cell, x0, y0 = tc.exp5()
    probes, kept = tc.exp5_probes()
    left = float((~kept).mean())
    assert left <= tc.MAX_LEFT_OUT
    probes = tc.Probes(np.array(probes.cx)[kept], np.array(probes.cy)[kept], probes.x[kept], probes.y[kept])
    entry = _eval(P, mode, probes, H[None], (cell, x0, y0), exact=False)
    entry["share_left_out"] = left
    tc.record("gpu_eval_" + MODE_NAME[mode], "exp5", entry)
    _assert_eval(entry, exact=False)


# ---- (b) k_plan_check, (c) k_force_fit on the sweep -------------------------------------------------------------------------------

def _sweep(P, cfg):
    """The sweep plans with what the statement says at the positions and forces Planner.sample returns."""
    plans, L = tc.sweep_plans()
    maps = tc.stack()
    t0 = 3.756 + 10.0 * np.arange(len(plans))
    mid = np.array(tc.SWEEP_MAP_ID, np.int32)
    P.set_heightfields(maps, *DYADIC)
    sample = P.sample(plans, t0, hz=tc.SWEEP_HZ, n_rows=tc.SWEEP_ROWS)
    return plans, L, maps, t0, mid, sample


def test_plan_check_samples_the_look_up_across_the_map(planner):
    from qtos_amd import capi, plan_check as pc
    mode, cfg, P = planner
    plans, L, maps, t0, mid, sample = _sweep(P, cfg)
    n, nx, ny = tc.SWEEP_ROWS, *tc.STACK_SHAPE
    rows, _ = P.plan_check(plans, t0, capi.check_params(hz=tc.SWEEP_HZ, n_rows=n, tol=pcc.TOL), map_id=mid)
    assert rows.shape == (len(plans), n, 27) and np.array_equal(rows[:, :, 0], sample[:, :, 0])
    stance = pc.stance_rows(L, tc.SWEEP_HZ, 0, n)
    t = np.minimum(np.arange(n) / tc.SWEEP_HZ, L.T)
    decided = np.ones(n, bool)                              # test_gpu_plan_check.py: further than 1e-9 s from a phase switch
    for e in range(4):
        for sw in pcc.node_times(L.splines[2 + e])[1:-1]:
            decided &= np.abs(t - sw) > 1e-9
    got_t, got_f, want, keep_t, keep_f = [], [], {LD: ([], []), F64: ([], [])}, [], []
    seen_x, seen_y = set(), set()
    for b in range(len(plans)):
        for e in range(4):
            p, f = sample[b, :, 7 + 3 * e:10 + 3 * e], sample[b, :, 25 + 3 * e:28 + 3 * e]
            fx, fy = ot.grid_coordinate(p[:, 0], tc.X0, tc.CELL), ot.grid_coordinate(p[:, 1], tc.Y0, tc.CELL)
            jump_h = (tc.near_line(fx, nx, "ties") | tc.near_line(fy, ny, "ties")) if mode == 1 else np.zeros(n, bool)
            jump_s = (tc.near_line(fx, nx, "lines") | tc.near_line(fy, ny, "lines")) if mode == 0 else np.zeros(n, bool)
            keep_t.append(~jump_h), keep_f.append(~jump_h & ~jump_s & decided)
            got_t.append(rows[b, :, 19 + e]), got_f.append(rows[b, :, 23 + e])
            for dt in (LD, F64):
                h, hx, hy, hxy = ot.lookup(maps[mid[b]], *DYADIC, p[:, 0], p[:, 1], mode, dt)
                want[dt][0].append(p[:, 2].astype(dt) - h)
                want[dt][1].append(tc.check_force_excess(ot.force_rows(f, hx, hy, hxy, cfg.friction, dt)[0], f, stance[:, e], cfg.force_limit, dt))
            seen_x |= set(np.array(tc.axis_class(fx.astype(F64), nx))[~jump_h])
            seen_y |= set(np.array(tc.axis_class(fy.astype(F64), ny))[~jump_h])
    keep_t, keep_f = np.array(keep_t), np.array(keep_f)
    entry = dict(rows=int(keep_t.size), terrain_left_out=float((~keep_t).mean()), force_left_out=float((~keep_f).mean()))
    for name, got, k, keep in (("terrain", got_t, 0, keep_t), ("force", got_f, 1, keep_f)):
        ref, f64 = np.array(want[LD][k]), np.array(want[F64][k])
        floor = tc.dist(f64[keep], ref[keep])
        entry[name] = dict(floor=floor, gate=pcc.gate(name, floor), err=tc.dist(np.array(got)[keep], ref[keep]), compared=int(keep.sum()))
    entry["classes_x"], entry["classes_y"] = sorted(seen_x), sorted(seen_y)
    tc.record("gpu_plan_check_" + MODE_NAME[mode], "sweep", entry)
    assert entry["terrain_left_out"] <= tc.MAX_LEFT_OUT
    assert seen_x >= tc.SWEEP_CLASSES_X and seen_y >= tc.SWEEP_CLASSES_Y
    assert entry["force"]["compared"] > keep_f.size // 4
    for name in ("terrain", "force"):
        assert entry[name]["err"] <= entry[name]["gate"], (name, entry[name])


def test_force_fit_on_the_sweep_matches_its_statement(planner):
    from qtos_amd import capi, force_fit as ff, plan_check as pc
    mode, cfg, P = planner
    plans, L, maps, t0, mid, sample = _sweep(P, cfg)
    n, nx, ny = tc.SWEEP_ROWS, *tc.STACK_SHAPE
    rows, status, _ = P.force_fit(plans, t0, capi.fit_params(cfg, hz=tc.SWEEP_HZ, n_rows=n, tol=ffc.TOL), map_id=mid)
    stance = pc.stance_rows(L, tc.SWEEP_HZ, 0, n)
    t = np.minimum(np.arange(n) / tc.SWEEP_HZ, L.T)
    decided = np.ones(n, bool)
    for e in range(4):
        for sw in pcc.node_times(L.splines[2 + e])[1:-1]:
            decided &= np.abs(t - sw) > 1e-9
    worst, compared = {}, 0
    for b in range(len(plans)):
        keep = decided.copy()
        if mode == 0:                                       # a stance foot on a line: its slopes, and with them the fit, are undecided
            for e in range(4):
                p = sample[b, :, 7 + 3 * e:10 + 3 * e]
                fx, fy = ot.grid_coordinate(p[:, 0], tc.X0, tc.CELL), ot.grid_coordinate(p[:, 1], tc.Y0, tc.CELL)
                keep &= ~(stance[:, e] & (tc.near_line(fx, nx, "lines") | tc.near_line(fy, ny, "lines")))
        compared += int(keep.sum())
        terrain = (maps[mid[b]],) + DYADIC
        (w_ld, _, _), (w_64, _, d_64) = (ff.fit_rows(L, plans[b], t0[b], tc.SWEEP_HZ, 0, n, cfg, ff.fit_params(cfg), terrain=terrain,
                                                     dtype=dt, detail=True) for dt in (LD, F64))
        groups = {g: c for g, c in ffc.GROUPS.items() if g != "tau"}
        for c, per in ffc.compare(rows[b], w_ld, w_64, d_64, groups=groups, rows=keep).items():
            for g, w in per.items():
                key = "stance_%d_%s" % (c, g)
                if key not in worst or w["err"] / w["gate"] > worst[key]["err"] / worst[key]["gate"]:
                    worst[key] = dict(w, window=b)
    tc.record("gpu_force_fit_" + MODE_NAME[mode], "sweep", dict(rows_compared=compared, rows=n * len(plans), **worst))
    assert compared >= (40 if mode == 0 else n * len(plans) * 99 // 100)
    for key, w in worst.items():
        assert w["err"] <= w["gate"], (key, w)


# ---- (c) the starting point and the shifted warm start ---------------------------------------------------------------------------

# goals in grid coordinates of the dyadic 5 x 7 grid: beyond a border, exactly on the last border lines, on a node, far
GOALS = ((-2.0, 8.0), (4.0, 6.0), (2.0, 3.0), (3e9, 2.25), (-3e9, 1e12))
FAR_GOALS = (3, 4)


def _goal_problems(cfg, mode, maps, mid):
    from oracle.oracle import Oracle, oracle_dict
    start, goal = sc.problems(len(GOALS), seed=83)
    goal[:, 0] = [tc.X0 + tc.CELL * g[0] for g in GOALS]
    goal[:, 1] = [tc.Y0 + tc.CELL * g[1] for g in GOALS]
    Os = [Oracle(oracle_dict(cfg), height=maps[m], hcell=tc.CELL, hx0=tc.X0, hy0=tc.Y0) for m in mid]
    qs = [sc.oracle_problem(O, cfg, s, g) for O, s, g in zip(Os, start, goal)]
    # what is under the goal and under the feet's nominal end points: the classes the look-up is met in
    seen = set()
    for g in goal:
        for d in [np.zeros(2)] + [np.asarray(cfg.nominal_stance)[e, 0:2] for e in range(4)]:
            seen.add(tc.axis_class([(g[0] + d[0] - tc.X0) / tc.CELL], tc.STACK_SHAPE[0])[0])
            seen.add(tc.axis_class([(g[1] + d[1] - tc.Y0) / tc.CELL], tc.STACK_SHAPE[1])[0])
    assert seen >= {"last_border", "node", "beyond_two_lo", "beyond_two_hi", "far_3e9_hi", "far_3e9_lo", "far_1e12_hi"}, seen
    return start, goal, Os, qs


def _line_error(L, got, want):
    """Largest error of a straight-line vector: the heights, which come from the look-up, absolutely; the rest relative to
    max(1, |value|) -- a far goal puts the line's x at 10^8 m, where an absolute 1e-12 is below a rounding."""
    z = (L.var_dim == 2) & (L.var_is_vel == 0) & (L.var_set != 1) & (L.var_set < 6)
    err = np.abs(got - want)
    return float(max(err[z].max(), (err / np.maximum(1.0, np.abs(want)))[~z].max()))


def test_starting_point_and_shifted_warm_start_read_the_look_up_at_its_edges(planner):
    from test_gpu_splines import _check_shift, _shift_reference
    mode, cfg, P = planner
    _, _, L = lc.case(tc.CASE)
    maps = tc.stack()
    mid = np.array([2, 0, 1, 2, 0], np.int32)
    start, goal, Os, qs = _goal_problems(cfg, mode, maps, mid)
    P.set_heightfields(maps, *DYADIC)
    got = P.initial_guess(start, goal, map_id=mid)
    line = np.array([O.initial_guess(q) for O, q in zip(Os, qs)])
    assert not Os[0].swing_start_on_rule
    lo_hi = [O.var_bounds(q) for O, q in zip(Os, qs)]
    entry = dict(initial_guess=[], shift_warm_behind_the_horizon=[])
    for b in range(len(GOALS)):
        fixed = lo_hi[b][0] == lo_hi[b][1]
        assert np.array_equal(got[b, fixed], lo_hi[b][0][fixed])
        entry["initial_guess"].append(_line_error(L, got[b], line[b]))
    # the heights do come from the maps, and from each window's own
    last_z = np.array([L.off_eem[e] + L.n_eem[e] - 1 for e in range(4)])
    assert len(np.unique(got[:, last_z])) > 8
    # k_shift_warm: everything behind the previous plan's horizon is the straight line; T - 0.3: most of it
    plans, _, _ = sc.random_plans(tc.CASE, len(GOALS), seed=51)
    out = P.shift_warm(plans, np.full(len(GOALS), 1e9), start, goal, map_id=mid)
    for b in range(len(GOALS)):
        entry["shift_warm_behind_the_horizon"].append(_line_error(L, out[b], line[b]))
    near = [b for b in range(len(GOALS)) if b not in FAR_GOALS]
    off = np.full(len(near), L.T - 0.3)
    out = P.shift_warm(plans[near], off, start[near], goal[near], map_id=mid[near])
    nlh, nline = [lo_hi[b] for b in near], line[near]
    ref, f64, inside = _shift_reference(L, plans[near], off, nlh, nline)
    vg = sc.var_groups(L)
    floor = {}
    for b in range(len(near)):
        floor = sc.merge_max(floor, sc.group_max((f64[b] - ref[b])[inside[b]], vg[inside[b]]))
    achieved = _check_shift(L, out, ref, inside, nlh, nline, "terrain edges")
    entry["shift_warm_floor"], entry["shift_warm_achieved"] = floor, achieved
    tc.record("gpu_line_" + MODE_NAME[mode], "goals", entry)
    assert max(entry["initial_guess"]) <= LINE_TOL and max(entry["shift_warm_behind_the_horizon"]) <= LINE_TOL
    sc.assert_within(achieved, floor, "k_shift_warm at the terrain's edges")


# ---- (c) the feedback hand-over ------------------------------------------------------------------------------------------------

FEEDBACK_HZ, FEEDBACK_CAP = 10.0, 6
FEEDBACK_ROWS = (3, 5, 2, 4, 6)
FEEDBACK_MAPS = (2, 0, 1, 3, -1)                          # 3 = n_maps and -1: clamped to the last and the first map
# (foot, fx, fy): where that foot of the window stands, in grid coordinates of the dyadic 5 x 7 grid -- every foot beyond the
# borders; on both last border lines; on a node; far (the other feet of a window stand within four cells of it)
FEEDBACK_TARGETS = ((0, -12.0, 20.0), (0, 4.0, 6.0), (3, 2.0, 3.0), (0, 3.1e9, 2.25), (0, -3.1e9, 1e12))


def test_start_feedback_snaps_the_feet_to_the_look_up_at_its_edges(planner):
    """k_start_feedback reads the height under every corrected foot.  Five windows of the straight-line plan from rest, moved so
    that the feet stand at FEEDBACK_TARGETS; the start vectors' feet are put on quarters of a cell exactly and the feet's gain is
    0, so the corrected feet are those coordinates to the bit and the snapped z must be the statement's h with ==.  The rest of
    the start vector and the status words against feedback.start_feedback with terrain_lookup in float64."""
    from qtos_amd import capi, feedback, workloads
    mode, cfg, P = planner
    _, O, L = lc.case(tc.CASE)
    maps = tc.stack()
    P.set_heightfields(maps, *DYADIC)
    B, hz, cap = len(FEEDBACK_ROWS), FEEDBACK_HZ, FEEDBACK_CAP
    rows, mid = np.array(FEEDBACK_ROWS, np.int32), np.array(FEEDBACK_MAPS, np.int32)
    s = workloads.rest_start(0.0)
    x = O.initial_guess(O.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), np.array([0.1, 0.0, 0.24])))
    t0 = 1.5 + np.arange(B)
    nodes = np.repeat(x[None], B, axis=0)
    first = P.sample(nodes, t0, hz=hz, n_rows=cap + 1)
    pos = (L.var_is_vel == 0) & np.isin(L.var_set, [0, 2, 3, 4, 5])
    for b, (f, fx, fy) in enumerate(FEEDBACK_TARGETS):
        nodes[b, pos & (L.var_dim == 0)] += tc.X0 + tc.CELL * fx - first[b, rows[b], 7 + 3 * f]
        nodes[b, pos & (L.var_dim == 1)] += tc.Y0 + tc.CELL * fy - first[b, rows[b], 8 + 3 * f]
    sample = P.sample(nodes, t0, hz=hz, n_rows=cap + 1)
    joint, _ = P.joint_rows(nodes, t0, capi.joint_params(hz=hz, n_rows=cap, tau_max=0.0))
    meas = np.concatenate([sample[:, :cap, 1:7], joint[:, :, 1:13]], axis=2)
    start = np.stack([sample[b, rows[b], 1:25] for b in range(B)])
    q = tc.CELL / 4
    for o, org in ((6, tc.X0), (7, tc.Y0)):                 # the feet's x and y on quarters of a cell
        cols = o + 3 * np.arange(4)
        moved = org + q * np.round((start[:, cols] - org) / q)
        assert np.abs(moved - start[:, cols]).max() <= q / 2 + 1e-7
        start[:, cols] = moved
    seen = set()
    for b, (f, fx, fy) in enumerate(FEEDBACK_TARGETS):
        gx, gy = (start[b, 6 + 3 * np.arange(4)] - tc.X0) / tc.CELL, (start[b, 7 + 3 * np.arange(4)] - tc.Y0) / tc.CELL
        if abs(fx) < 1e9:
            assert gx[f] == fx and gy[f] == fy
        seen |= set(tc.axis_class(gx, tc.STACK_SHAPE[0])) | set(tc.axis_class(gy, tc.STACK_SHAPE[1]))
    assert seen >= {"last_border", "node", "beyond_two_lo", "beyond_two_hi", "far_3e9_hi", "far_3e9_lo", "far_1e12_hi"}, seen
    params = capi.feedback_params(cfg, hz=hz, n_rows=cap, gain_pos=0.75, gain_ang=0.75, gain_foot=0.0)
    got, _, err, status = P.start_feedback(nodes, t0, rows, meas, params, start, map_id=mid)
    look = feedback.terrain_lookup(maps, tc.CELL, tc.X0, tc.Y0, mode)
    want, _, _, want_status = feedback.start_feedback_batch(L, nodes, t0, rows, meas, params, start, look, mid, None, None, F64)
    unequal, worst = 0, 0.0
    for b in range(B):
        m = min(max(int(mid[b]), 0), len(maps) - 1)
        fx_, fy_ = start[b, 6 + 3 * np.arange(4)], start[b, 7 + 3 * np.arange(4)]
        assert np.array_equal(got[b, 6 + 3 * np.arange(4)], fx_) and np.array_equal(got[b, 7 + 3 * np.arange(4)], fy_)
        h64, h_ld = (ot.lookup(maps[m], *DYADIC, fx_, fy_, mode, dt)[0] for dt in (F64, LD))
        assert np.array_equal(h64.astype(LD), h_ld)
        unequal += int((got[b, 8 + 3 * np.arange(4)] != h64).sum())
        worst = max(worst, float((np.abs(got[b] - want[b]) / np.maximum(1.0, np.abs(want[b]))).max()))
    entry = dict(windows=B, snapped_z_unequal=unequal, status=[int(v) for v in status], status_of_the_rule=[int(v) for v in want_status],
                 rest_of_the_start_vector=worst, gate=LINE_TOL, classes=sorted(seen))
    tc.record("gpu_start_feedback_" + MODE_NAME[mode], "targets", entry)
    assert np.array_equal(status, want_status)
    assert all(int(v) & feedback.CORRECTED and not int(v) & feedback.FALLBACK for v in status)       # the look-up was read
    assert any(int(v) & (0xF * feedback.SNAPPED) for v in status)
    assert unequal == 0 and worst <= LINE_TOL
