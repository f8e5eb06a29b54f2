"""The three kernels that turn a node vector into numbers through the cubic-Hermite splines -- k_sample, k_shift_warm and
the starting-point code (initial_value / straight_line_value / table_value through k_debug_guess) -- against
oracle/splines.py, the numpy restatement of the spline layer in longdouble, on six transcriptions and random plans.

Gates of the spline checks (nothing is fixed in advance): a check compares the GPU with the longdouble restatement; its
gate is the error of the same formulas in plain float64 on the same inputs, measured here on the CPU -- for k_sample
max |oracle.sample - longdouble|, for k_shift_warm max |shift_warm(float64) - longdouble| --, per group (motion values,
motion velocities, force values, force derivatives) over all inputs of the transcription, times 8 and never above 1e-10.
The 8 covers the kernel's cumulative end-time table (the CPU code subtracts the durations one by one: the local time is
rounded differently) and the device build's contraction of multiply-adds; the cap keeps an inflated floor from hiding a
failure.  A wrong index, node time or segment is an error of order 0.1 (20 N on the forces).  Floors and achieved errors
are printed and, where QTOS_SPLINE_ACCURACY names a file, kept in it (profiles/spline_accuracy.json is one such run).

Variables that come from the straight line (behind the previous plan's horizon; the starting point) are held to the
oracle's straight-line guess at 1e-12, the gate test_nominal_plan_table_as_starting_point has had for it; fixed variables
carry the problem's data to the bit."""
import numpy as np
import pytest

import spline_cases as sc
from oracle import splines as sp

pytestmark = pytest.mark.gpu

LINE_TOL = 1e-12
_planners = {}


@pytest.fixture(scope="module")
def planner():
    """planner(name): the one Planner of a transcription (max_batch 8), created at its first use, closed with the module."""
    from qtos_amd.capi import Planner

    def get(name):
        if name not in _planners:
            _planners[name] = Planner(sc.case(name)[0], max_batch=8)
        return _planners[name]
    yield get
    for P in _planners.values():
        P.close()
    _planners.clear()


def _offsets(L):
    """The five shifts: none; off every grid; most variables behind the horizon; one base node exactly on the horizon (the
    <= T + 1e-9 edge); everything behind the horizon."""
    k = L.n_base_nodes // 2
    edge = L.T - L.splines[0].node_times()[k]
    assert abs((edge + L.splines[0].node_times()[k]) - L.T) < 1e-12
    return np.array([0.0, 0.5 * L.T + 0.0137, L.T - 0.3, edge, 1e9])


def _shift_reference(L, plans, off, lo_hi, line):
    """(longdouble reference, float64 form, mask of the variables read from the previous plan) of a batch."""
    ref, f64, inside = [], [], []
    for b in range(len(plans)):
        lo, hi = lo_hi[b]
        fixed = lo == hi
        # (input condition: no node time within 1e-11 of the horizon's threshold, where float64 and longdouble could part)
        assert np.abs(off[b] + L.node_time - (L.T + sp.HORIZON_EPS)).min() > 1e-11
        ref.append(sp.shift_warm(L, plans[b], off[b], fixed, lo, line[b], np.longdouble))
        f64.append(sp.shift_warm(L, plans[b], off[b], fixed, lo, line[b], np.float64))
        inside.append(sp.shifted_mask(L, off[b], fixed))
    return np.array(ref), np.array(f64), np.array(inside)


def _shift_problem_set(name, oracles=None, map_id=None, goal_xy=None):
    """Previous plans, new starts / goals, the oracle's bounds and straight-line guesses of the B = 5 problems."""
    cfg, O, L = sc.case(name)
    plans, _, _ = sc.random_plans(name, 5, seed=51)
    start, goal = sc.problems(5, seed=52)
    if goal_xy is not None:
        goal[:, 0:2] = goal_xy
    Os = [O] * 5 if oracles is None else [oracles[m] for m in map_id]
    qs = [sc.oracle_problem(Os[b], cfg, start[b], goal[b]) for b in range(5)]
    lo_hi = [Os[b].var_bounds(qs[b]) for b in range(5)]
    line = np.array([Os[b].initial_guess(qs[b]) for b in range(5)])
    return plans, start, goal, lo_hi, line


def _identity_caps(L, plans):
    """What the gate of the offset-0 identity may at most be, per group.  That check compares the kernel with the previous
    plan itself, not with the restatement at the same float64 time, so the rounding of the node time counts: a float64
    sum of up to n_polys durations, off the exact node by at most n_polys eps T / 2, plus eps T for the evaluation's own
    local time.  At a node the value weights are flat (second order: the spline checks' cap of 1e-10 stays); the
    derivative weights have the slope 6 / T_poly^2 there, on node values at most 2 max |value| apart."""
    eps = np.finfo(np.float64).eps
    caps = {}
    for g, sets in ((1, range(0, 6)), (3, range(6, 10))):
        slope = max((L.splines[s].n_polys / 2 + 1) * eps * L.T * 6.0 / L.splines[s].dur.min() ** 2 for s in sets)
        values = np.abs(plans[:, (L.var_is_vel == 0) & np.isin(L.var_set, list(sets))]).max()
        caps[sc.GROUPS[g]] = slope * 2.0 * values
    caps[sc.GROUPS[0]] = caps[sc.GROUPS[2]] = sc.GATE_CAP
    return caps


def _check_shift(L, out, ref, inside, lo_hi, line, what):
    """Fixed variables to the bit, straight-line variables to 1e-12; returns the error of the spline variables per group."""
    vg = sc.var_groups(L)
    worst = {}
    for b in range(len(out)):
        lo, hi = lo_hi[b]
        fixed = lo == hi
        assert np.array_equal(out[b, fixed], lo[fixed]), what
        behind = ~fixed & ~inside[b]
        if behind.any():
            assert np.abs(out[b, behind] - line[b, behind]).max() <= LINE_TOL, what
        if inside[b].any():
            worst = sc.merge_max(worst, sc.group_max((out[b] - ref[b])[inside[b]], vg[inside[b]]))
    return worst


@pytest.mark.parametrize("name", sc.NAMES)
def test_shift_warm_matches_the_restatement(planner, name):
    """k_shift_warm on B = 5 previous plans, new starts and goals, five offsets: every problem is shifted by every offset
    (five calls, the offsets rotated through the batch) and compared with oracle/splines.shift_warm in longdouble --
    fixed values the oracle's lo of the new problem, the straight line the oracle's initial_guess (the kernel does not
    apply the swing rule).

    Properties: offset 0 returns the previous plan on the free variables (the check that catches node times taken from
    the elimination order's keys: a foothold in front of a swing then gets the NEXT foothold's position, an error of
    order 0.1); the 1e9 row is the oracle's initial_guess to 1e-12; non-zero start velocities are ignored by a
    configuration that does not honour them and carried by the one that does; every row of a B = 5 call is bit-equal to
    the B = 1 call of that problem; the device form on torch tensors is bit-equal to the host form."""
    import torch
    cfg, O, L = sc.case(name)
    P = planner(name)
    assert P.n == L.n_vars and P.dims.duration == L.T
    plans, start, goal, lo_hi, line = _shift_problem_set(name)
    offsets = _offsets(L)
    vg = sc.var_groups(L)
    vel = np.concatenate([L.off_lin + 3 + np.arange(3), L.off_ang + 3 + np.arange(3)])
    assert (start[:, 18:24] != 0).all()
    floor, achieved, identity, identity_floor = {}, {}, {}, {}
    for r in range(5):
        off = np.roll(offsets, r)
        out = P.shift_warm(plans, off, start, goal)
        ref, f64, inside = _shift_reference(L, plans, off, lo_hi, line)
        for b in range(5):
            floor = sc.merge_max(floor, sc.group_max((f64[b] - ref[b])[inside[b]], vg[inside[b]]) if inside[b].any() else {})
        achieved = sc.merge_max(achieved, _check_shift(L, out, ref, inside, lo_hi, line, "%s, rotation %d" % (name, r)))
        for b in range(5):
            fixed = lo_hi[b][0] == lo_hi[b][1]
            if cfg.honor_start_velocity:
                assert np.array_equal(out[b, vel], start[b, 18:24])
            else:
                assert np.array_equal(out[b, vel], np.zeros(6))
            if off[b] == 0.0:
                assert inside[b][~fixed].all()
                identity = sc.merge_max(identity, sc.group_max((out[b] - plans[b])[~fixed], vg[~fixed]))
                for form in (f64[b], ref[b]):
                    identity_floor = sc.merge_max(identity_floor, sc.group_max((form - plans[b].astype(np.longdouble))[~fixed], vg[~fixed]))
            if off[b] == 1e9:
                assert not inside[b].any() and np.abs(out[b] - line[b]).max() <= LINE_TOL
            if off[b] == offsets[3]:    # the edge: the base node on the horizon is read from the plan, the next one is not
                k = L.n_base_nodes // 2
                assert inside[b][L.off_lin + 6 * k + 2] and not inside[b][L.off_lin + 6 * (k + 1) + 2]
        if r == 0:
            for b in range(5):
                one = P.shift_warm(plans[b:b + 1], off[b:b + 1], start[b:b + 1], goal[b:b + 1])
                assert np.array_equal(one[0], out[b])
            dev = [torch.tensor(a, dtype=torch.float64, device="cuda") for a in (plans, off, start, goal)]
            warm = torch.full((5, P.n), float("nan"), dtype=torch.float64, device="cuda")
            rc = P.lib.qtos_shift_warm_device(P.h, 5, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), None,
                                              warm.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
            torch.cuda.synchronize()
            assert np.array_equal(warm.cpu().numpy(), out)
    sc.record("k_shift_warm", name, floor, achieved)
    sc.record("k_shift_warm_identity", name, identity_floor, identity)
    sc.assert_within(achieved, floor, "k_shift_warm [%s]" % name)
    # the identity: 8 x what the restatement itself leaves of it -- the larger of its two forms: the longdouble one evaluates
    # exactly AT the float64 node time and so shows the rounding of that time, which the float64 form's one-by-one subtraction
    # of the durations it was summed from partly cancels --, never above the bound the rounding of a node time explains
    caps = _identity_caps(L, plans)
    assert max(caps.values()) < 1e-6, caps
    for k, v in identity.items():
        assert v <= min(sc.GATE_FACTOR * identity_floor[k], caps[k]), (name, k, v, identity_floor[k], caps[k])


def test_shift_warm_reads_the_terrain_of_each_problems_own_map(planner):
    """The 200-knot transcription on the randomized heightfields, a different map per problem: the variables behind the
    previous plan's horizon carry the terrain height of THEIR map -- one Oracle(height = maps[m]) per map."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    name = "knots200_vel"
    cfg, _, L = sc.case(name)
    P = planner(name)
    maps, cell = workloads.random_terrains()
    map_id = np.array([3, 0, 7, 5, 2], np.int32)
    oracles = {int(m): Oracle(oracle_dict(cfg), height=maps[m], hcell=cell) for m in map_id}
    # (goals on the ledges, x in 0.4 .. 1.5, where the maps' levels differ; the flat floor in front of them is 0 on every map)
    rng = np.random.default_rng(53)
    goal_xy = np.stack([rng.uniform(0.65, 1.25, 5), rng.uniform(-0.3, 0.3, 5)], axis=1)
    plans, start, goal, lo_hi, line = _shift_problem_set(name, oracles, [int(m) for m in map_id], goal_xy)
    _assert_off_the_cell_edges(cfg, maps.shape[1:], cell, goal, mode=1)
    off = np.array([L.T - 0.3, 1e9, 0.5 * L.T + 0.0137, 1e9, L.T - 0.3])
    vg = sc.var_groups(L)
    P.set_heightfields(maps, cell)
    try:
        out = P.shift_warm(plans, off, start, goal, map_id=map_id)
    finally:
        P.set_heightfields(None, cell)
    ref, f64, inside = _shift_reference(L, plans, off, lo_hi, line)
    floor = {}
    for b in range(5):
        floor = sc.merge_max(floor, sc.group_max((f64[b] - ref[b])[inside[b]], vg[inside[b]]) if inside[b].any() else {})
    achieved = _check_shift(L, out, ref, inside, lo_hi, line, "terrain")
    sc.record("k_shift_warm", name + "_random_terrains", floor, achieved)
    sc.assert_within(achieved, floor, "k_shift_warm on terrain")
    # the inputs tell the maps apart: the straight line of a neighbour's map is off by millimetres
    for b in range(5):
        other = oracles[int(map_id[(b + 1) % 5])]
        wrong = other.initial_guess(sc.oracle_problem(other, cfg, start[b], goal[b]))
        behind = ~(lo_hi[b][0] == lo_hi[b][1]) & ~inside[b]
        assert np.abs(wrong - line[b])[behind].max() > 1e-4


@pytest.mark.parametrize("name", sc.NAMES)
def test_sampler_matches_the_restatement_on_random_plans(planner, name):
    """k_sample on B = 3 random plans with distinct t0, at 1000 Hz and 400 Hz, round(T hz) + 8 rows (the rows past the
    horizon hold the state at T with the clock running on), and with 1 row and 257 rows (one row into the second
    workgroup): against oracle/splines.sample_rows in longdouble at the gate derived from |oracle.sample - longdouble|,
    against oracle.sample at that gate plus the floor (the triangle inequality), the time stamps to the bit; every batch
    row bit-equal to its B = 1 call."""
    cfg, O, L = sc.case(name)
    P = planner(name)
    plans, _, _ = sc.random_plans(name, 3, seed=61)
    t0 = np.array([0.0, 1.25, 7.5])
    rg = sc.row_groups()
    floor, achieved, vs_oracle = {}, {}, {}
    for hz, n_rows in [(1000.0, None), (400.0, None), (1000.0, 1), (1000.0, 257)]:
        full = n_rows is None
        n_rows = int(round(L.T * hz)) + 8 if full else n_rows
        rows = P.sample(plans, t0, hz=hz, n_rows=n_rows)
        assert rows.shape == (3, n_rows, 37)
        for b in range(3):
            ro = O.sample(plans[b], t0=t0[b], hz=hz, n_rows=n_rows)
            rl = sp.sample_rows(L, plans[b], t0[b], hz, n_rows, np.longdouble)
            assert np.array_equal(rows[b, :, 0], t0[b] + np.arange(n_rows) / hz) and np.array_equal(rows[b, :, 0], ro[:, 0])
            floor = sc.merge_max(floor, sc.group_max(ro - rl, rg))
            achieved = sc.merge_max(achieved, sc.group_max(rows[b] - rl, rg))
            vs_oracle = sc.merge_max(vs_oracle, sc.group_max(rows[b] - ro, rg))
            if full:    # the last 7 rows lie past the horizon
                assert np.array_equal(rows[b, -6:, 1:], np.repeat(rows[b, -7:-6, 1:], 6, 0)) and np.all(np.diff(rows[b, -9:, 0]) > 0)
                assert np.abs(rows[b, -9, 1:] - rows[b, -8, 1:]).max() > 1e-6
        if hz == 400.0 or n_rows == 257:
            for b in range(3):
                assert np.array_equal(P.sample(plans[b:b + 1], t0[b:b + 1], hz=hz, n_rows=n_rows)[0], rows[b])
    sc.record("k_sample", name, floor, dict(achieved, **{"vs_oracle_" + k: v for k, v in vs_oracle.items()}))
    sc.assert_within(achieved, floor, "k_sample [%s]" % name)
    g = sc.gates(floor)
    for k, v in vs_oracle.items():
        assert v <= g[k] + floor[k], (name, k, v, g[k], floor[k])


# ---- starting point ---------------------------------------------------------------------------------------------------
def _assert_off_the_cell_edges(cfg, shape, cell, goal, mode, x0=-1.0, y0=-1.0, tol=1e-6):
    """Input condition of the terrain checks: neither a goal nor a foot's nominal end point lies within 1e-6 of a cell edge
    (nearest-cell lookup) or of the map's border (clamping) -- the device build may contract (x - x0) / cell + 0.5
    differently from the host, and a flipped cell there is not a finding.  Asserted, never skipped."""
    pts = [goal[:, 0:2]] + [goal[:, 0:2] + np.asarray(cfg.nominal_stance)[e, 0:2] for e in range(4)]
    for p in pts:
        for f, n in (((p[:, 0] - x0) / cell, shape[0]), ((p[:, 1] - y0) / cell, shape[1])):
            if mode == 1:
                h = f + 0.5
                assert (np.abs(h - np.round(h)) * cell > tol).all()
            assert (np.abs(f) * cell > tol).all() and (np.abs(f - (n - 1)) * cell > tol).all()


def _terrain_problems(cfg, n, seed):
    """Starts and goals over the stepped part of the maps (x in [-1, 2.99], y in [-1, 0.99]); the goal of problem n - 2 lies
    outside the heightfield (clamped), the front feet's nominal end points of problem n - 1 do (its goal does not)."""
    start, _ = sc.problems(n, seed)
    rng = np.random.default_rng(seed + 7)
    goal = np.stack([rng.uniform(0.25, 2.6, n), rng.uniform(-0.4, 0.4, n), np.full(n, 0.24)], axis=1)
    goal[n - 2, 0:2] = [3.4137, 0.1]
    goal[n - 1, 0:2] = [2.9, 0.3]
    return start, goal


def _guess_vs_oracle(P, cfg, oracles, start, goal, map_id):
    got = P.initial_guess(start, goal, map_id=map_id)
    worst = 0.0
    for b in range(len(start)):
        O = oracles[int(map_id[b]) if map_id is not None else 0]
        want = O.start_point(sc.oracle_problem(O, cfg, start[b], goal[b]))
        lo, hi = O.var_bounds(sc.oracle_problem(O, cfg, start[b], goal[b]))
        assert np.array_equal(got[b, lo == hi], lo[lo == hi])
        worst = max(worst, float(np.abs(got[b] - want).max()))
    return got, worst


@pytest.mark.parametrize("name", sc.NAMES)
def test_starting_point_on_flat_ground_matches_the_oracle(planner, name):
    """Planner.initial_guess (k_debug_guess: initial_value / straight_line_value and, with reduce_swing, the swing rule) on
    B = 8 seeded problems with non-nominal stances and non-zero start velocities, against oracle.start_point: 1e-12."""
    cfg, O, L = sc.case(name)
    start, goal = sc.problems(8, seed=71)
    got, worst = _guess_vs_oracle(planner(name), cfg, {0: O}, start, goal, None)
    print("starting point, flat [%s]: worst |gpu - oracle| %.2e" % (name, worst))
    assert worst <= LINE_TOL
    vel = np.concatenate([L.off_lin + 3 + np.arange(3), L.off_ang + 3 + np.arange(3)])
    assert np.array_equal(got[:, vel], start[:, 18:24] if cfg.honor_start_velocity else np.zeros((8, 6)))


@pytest.mark.parametrize("terrain", ["random_terrains", "exp5_terrain"])
@pytest.mark.parametrize("name", ["knots100_trot", "knots200_vel"])
def test_starting_point_on_nearest_cell_terrain_matches_the_oracle(planner, name, terrain):
    """terrain_at under the goal and under each foot's nominal end point, nearest-cell lookup, per-problem map_id: the eight
    randomized maps (a different one per problem) and the exp_5 map; one goal outside the heightfield, one problem whose
    front feet end outside it."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    cfg, _, L = sc.case(name)
    assert cfg.terrain_mode == 1
    P = planner(name)
    if terrain == "random_terrains":
        maps, cell = workloads.random_terrains()
        map_id = np.array([5, 2, 7, 0, 3, 6, 1, 4], np.int32)
    else:
        m, cell = workloads.exp5_terrain()
        maps, map_id = m[None], np.zeros(8, np.int32)
    start, goal = _terrain_problems(cfg, 8, seed=81)
    _assert_off_the_cell_edges(cfg, maps.shape[1:], cell, goal, mode=1)
    x_max, nominal = -1.0 + (maps.shape[1] - 1) * cell, np.asarray(cfg.nominal_stance)
    assert goal[6, 0] > x_max + 0.1 and goal[7, 0] < x_max - 0.05 and goal[7, 0] + nominal[0, 0] > x_max + 0.05
    oracles = {int(m): Oracle(oracle_dict(cfg), height=maps[m], hcell=cell) for m in set(map_id.tolist())}
    P.set_heightfields(maps, cell)
    try:
        got, worst = _guess_vs_oracle(P, cfg, oracles, start, goal, map_id)
        flat = P.initial_guess(start, goal)     # (map 0 for every problem)
    finally:
        P.set_heightfields(None, cell)
    print("starting point, %s [%s]: worst |gpu - oracle| %.2e" % (terrain, name, worst))
    assert worst <= LINE_TOL
    # the inputs see the terrain, and where the maps differ, the map: the final foot heights differ by millimetres
    last_z = [L.off_eem[e] + L.n_eem[e] - 1 for e in range(4)]
    assert np.abs(got[:, last_z]).max() > 0.02
    if terrain == "random_terrains":
        assert np.abs(got - flat)[map_id != 0].max() > 1e-3


def test_starting_point_on_bilinear_terrain_matches_the_oracle():
    """The bilinear lookup (terrain_mode 0, every row of the reference's NLP kept) on the exp_5 map, clamped outside it."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.reference_compat(terrain_mode=0, reduce_base=False)
    m, cell = workloads.exp5_terrain()
    start, goal = _terrain_problems(cfg, 8, seed=91)
    _assert_off_the_cell_edges(cfg, m.shape, cell, goal, mode=0)
    O = Oracle(oracle_dict(cfg), height=m, hcell=cell)
    assert not O.swing_start_on_rule
    P = Planner(cfg, max_batch=8)
    try:
        P.set_heightfields(m[None], cell)
        got, worst = _guess_vs_oracle(P, cfg, {0: O}, start, goal, np.zeros(8, np.int32))
    finally:
        P.close()
    print("starting point, bilinear exp_5: worst |gpu - oracle| %.2e" % worst)
    assert worst <= LINE_TOL
    L = sp.layout(cfg)
    last_z = np.array([L.off_eem[e] + L.n_eem[e] - 1 for e in range(4)])
    hz = got[:, last_z]
    # (heights between the grid's levels: the interpolation is at work)
    levels = np.unique(m)
    assert (np.abs(hz[..., None] - levels).min(axis=-1) > 1e-5).any()


def test_nominal_plan_table_interpolation_matches_the_restatement(planner):
    """table_cell / table_value with a synthetic 3 x 2 table of seeded random node vectors (no solves) on the reference's
    walk: goals inside a cell, exactly on a grid line in x and in y, outside the grid on each of its four sides (clamped
    weights), all from non-nominal start stances and heights -- against oracle/splines.table_guess in longdouble followed
    by the oracle's swing rule.  Gate as for the spline checks: 8 x max |the same in float64 - longdouble| per group, at
    most 1e-10.  A 1 x 1 table is accepted (the i1 = i0, wx = 0 branch) and returns its one plan shifted to the start;
    set_init_table() afterwards restores the straight-line guess bit for bit."""
    name = "walk"
    cfg, O, L = sc.case(name)
    P = planner(name)
    assert O.swing_start_on_rule
    rng = np.random.default_rng(101)
    dx, dy = np.array([0.2, 0.5, 0.9]), np.array([-0.125, 0.125])
    sigma = np.where(L.var_set >= 6, sc.NOISE_FORCE, 1.0)
    nodes = rng.normal(size=(2, 3, L.n_vars)) * sigma
    start, goal = sc.problems(8, seed=102)
    start[1, 0], start[2, 1] = 0.5, 0.25            # (binary fractions: the displacements below are exact)
    disp = np.array([[0.31, 0.02], [0.5, -0.03], [0.7, 0.125], [0.1, 0.0], [1.3, 0.05], [0.4, -0.4], [0.6, 0.3], [0.83, -0.11]])
    goal[:, 0:2] = start[:, 0:2] + disp
    gx, gy = goal[:, 0] - start[:, 0], goal[:, 1] - start[:, 1]
    assert gx[1] == dx[1] and gy[2] == dy[1]                                    # exactly on a grid line
    assert gx[3] < dx[0] and gx[4] > dx[2] and gy[5] < dy[0] and gy[6] > dy[1]  # outside, each side
    for g, grid in ((gx, dx), (gy, dy)):   # (input condition: on a grid line exactly or not within 1e-6 of one)
        d = np.abs(g[:, None] - grid[None])
        assert ((d == 0) | (d > 1e-6)).all()
    before = P.initial_guess(start, goal)
    vg = sc.var_groups(L)

    def check(tdx, tdy, tnodes, what):
        P.set_init_table(tdx, tdy, tnodes)
        got = P.initial_guess(start, goal)
        floor, achieved = {}, {}
        for b in range(8):
            ref = O.project_swings(sp.table_guess(tdx, tdy, tnodes, start[b], goal[b], L, np.longdouble).astype(np.float64))
            f64 = O.project_swings(sp.table_guess(tdx, tdy, tnodes, start[b], goal[b], L, np.float64))
            fixed = L.fix_src >= 0
            assert np.array_equal(got[b, fixed], sp.fixed_values(L, start[b], goal[b])[1][fixed])
            floor = sc.merge_max(floor, sc.group_max(f64 - ref, vg))
            achieved = sc.merge_max(achieved, sc.group_max(got[b] - ref, vg))
        sc.record("table", what, floor, achieved)
        sc.assert_within(achieved, floor, "table guess, " + what)
        return got

    try:
        got = check(dx, dy, nodes, "3x2")
        assert np.abs(got - before).max() > 0.1             # (the table is in use)
        one = check(dx[1:2], dy[0:1], nodes[0:1, 1:2], "1x1")
        assert np.abs(one - got).max() > 0.1
    finally:
        P.set_init_table()
    assert np.array_equal(P.initial_guess(start, goal), before)
