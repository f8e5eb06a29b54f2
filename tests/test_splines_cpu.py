"""oracle/splines.py -- the numpy restatement of the spline layer the GPU tests of test_gpu_splines.py hold k_sample,
k_shift_warm and the starting-point code to -- against the C oracle and against itself.  No GPU."""
import numpy as np
import pytest

import spline_cases as sc
from oracle import splines as sp


@pytest.mark.parametrize("name", sc.NAMES)
def test_layout_agrees_with_the_oracle(name):
    """Sizes and offsets are the oracle's QoLayout; the variables the oracle fixes (lo == hi of var_bounds) are exactly the
    ones the layout's descriptors call start / goal / zero, with the values the descriptors name."""
    cfg, O, L = sc.case(name)
    assert L.n_vars == O.L.n_vars and L.n_base_nodes == O.L.n_base_nodes and L.T == O.L.T
    assert (L.off_lin, L.off_ang) == (O.L.off_lin, O.L.off_ang)
    assert L.off_eem == list(O.L.off_eem) and L.off_eef == list(O.L.off_eef)
    assert L.n_eem == list(O.L.n_eem) and L.n_eef == list(O.L.n_eef)
    start, goal = sc.problems(2, seed=21)
    for s, g in zip(start, goal):
        lo, hi = O.var_bounds(sc.oracle_problem(O, cfg, s, g))
        mask, val = sp.fixed_values(L, s, g)
        assert np.array_equal(mask, lo == hi)
        assert np.array_equal(val[mask], lo[mask])
    # the start velocities are fixed variables either way: carried where the configuration honours them, zero elsewhere
    vel = np.concatenate([L.off_lin + 3 + np.arange(3), L.off_ang + 3 + np.arange(3)])
    assert (start[:, 18:24] != 0).all()
    assert np.array_equal(L.fix_src[vel], 18 + np.arange(6) if cfg.honor_start_velocity else np.full(6, sp.FIX_ZERO))
    # every spline covers the horizon, every variable has one descriptor
    for S in L.splines:
        assert abs(S.dur.sum() - L.T) < 1e-12 and (S.dur > 0).all()
    assert np.array_equal(np.sort(np.unique(np.concatenate([S.idx[S.idx >= 0] for S in L.splines]))), np.arange(L.n_vars))


def test_the_fifth_transcription_has_a_short_last_base_polynomial():
    _, _, L = sc.case("short_last_poly")
    d = L.splines[0].dur
    assert len(d) == 13 and np.array_equal(d[:12], np.full(12, 0.2)) and abs(d[12] - 0.1) < 1e-12
    assert sc.case("two_base_polys")[2].n_base_nodes == 3


@pytest.mark.parametrize("name", sc.NAMES)
def test_sample_rows_agree_with_the_oracle(name):
    """sample_rows in longdouble against oracle.sample on random plans, at 1000 Hz and 400 Hz with 8 rows past the horizon:
    what separates the two is the float64 rounding of the oracle (this IS the floor the GPU gates are derived from, so here
    it is recorded and only held to the cap of those gates), and the float64 form of sample_rows is as close."""
    cfg, O, L = sc.case(name)
    plans, _, _ = sc.random_plans(name, 2, seed=31)
    rg = sc.row_groups()
    worst = {}
    for b, (hz, t0) in enumerate([(1000.0, 0.0), (400.0, 3.7)]):
        n_rows = int(round(L.T * hz)) + 8
        ro = O.sample(plans[b], t0=t0, hz=hz, n_rows=n_rows)
        rl = sp.sample_rows(L, plans[b], t0, hz, n_rows, np.longdouble)
        r64 = sp.sample_rows(L, plans[b], t0, hz, n_rows, np.float64)
        assert np.abs(ro[:, 0] - rl[:, 0]).max() <= 1e-15 * max(1.0, t0 + n_rows / hz)
        assert np.abs(np.asarray(ro[:, 1:], np.longdouble)).max() > 10.0           # (the forces: values of order 20 - 80)
        worst = sc.merge_max(worst, sc.group_max(ro - rl, rg))
        worst = sc.merge_max(worst, sc.group_max(r64 - rl, rg))
        # the last 7 rows lie past the horizon: the state at T, the clock running on (the row in front of them is the one
        # at round(T hz) / hz, which is T only to rounding)
        assert np.array_equal(ro[-6:, 1:], np.repeat(ro[-7:-6, 1:], 6, 0)) and np.array_equal(rl[-6:, 1:], np.repeat(rl[-7:-6, 1:], 6, 0))
        assert np.abs(ro[-8, 1:] - ro[-7, 1:]).max() < 1e-11 and np.abs(ro[-9, 1:] - ro[-8, 1:]).max() > 1e-6
        assert np.all(np.diff(ro[-9:, 0]) > 0)
    print("spline floor on the CPU [%s]: %s" % (name, worst))
    assert max(worst.values()) <= sc.GATE_CAP, worst


@pytest.mark.parametrize("name", sc.NAMES)
def test_node_times_are_where_the_unit_vectors_are_one(name):
    """For every variable v: the spline of its set, derivative is_vel[v], of the unit vector e_v at node_time[v] is 1 in
    component dim[v] -- the descriptors and the node times belong together.

    Bound: the arithmetic is longdouble, so what is left is the float64 rounding of the node time itself, a sum of up to
    n_polys durations: at most n_polys eps T.  At a node the value weights are flat and the derivative weights have the
    slope 6 / T_poly^2 (-6 tau / T^2 + 6 tau^2 / T^3 at tau = T_poly), so the error is at most n_polys eps T 6 / min(dur)^2:
    1e-9 on the 200 base polynomials of 0.05 s; a wrong node, set or time is an error of order 1."""
    _, _, L = sc.case(name)
    eps = np.finfo(np.float64).eps
    for s in range(sp.N_SETS):
        S = L.splines[s]
        tol = 1e-15 + S.n_polys * eps * L.T * 6.0 / S.dur.min() ** 2
        assert tol < 1e-8
        for q in range(2):
            vs = np.nonzero((L.var_set == s) & (L.var_is_vel == q))[0]
            if not len(vs):
                continue
            e = np.zeros((len(vs), L.n_vars))
            e[np.arange(len(vs)), vs] = 1.0
            out = sp.eval_spline(L, s, e, L.node_time[vs], q, np.longdouble)
            want = np.zeros((len(vs), 3))
            want[np.arange(len(vs)), L.var_dim[vs]] = 1.0
            assert np.abs(out - want).max() < tol, (s, q)
    for S in L.splines:
        assert np.array_equal(S.node_times()[1:], np.cumsum(S.dur))


@pytest.mark.parametrize("name", sc.NAMES)
def test_shift_warm_by_nothing_is_the_plan_and_by_everything_the_straight_line(name):
    """offset 0 with the plan's own fixed values returns the plan on its free variables, within 8 x the rounding floor
    (|float64 - longdouble| of the same call, per group); offset 1e9 returns the straight line.  The floors are printed:
    the force derivatives have by far the largest -- a force polynomial of a short stance lasts 12 .. 60 ms, its derivative
    weights have the slope 6 / T_poly^2 = 1.6e3 .. 4e4 per second at a node, and the node values differ by tens of newtons,
    so one ulp of the node time (1e-15) is 1e-10 N/s."""
    cfg, O, L = sc.case(name)
    plans, start, goal = sc.random_plans(name, 2, seed=41)
    vg = sc.var_groups(L)
    worst = {}
    for b in range(2):
        mask, _ = sp.fixed_values(L, start[b], goal[b])
        line = O.initial_guess(sc.oracle_problem(O, cfg, start[b], goal[b]))
        free = ~mask
        ref = sp.shift_warm(L, plans[b], 0.0, mask, plans[b], line, np.longdouble)
        f64 = sp.shift_warm(L, plans[b], 0.0, mask, plans[b], line, np.float64)
        assert sp.shifted_mask(L, 0.0, mask)[free].all()
        floor = sc.group_max(f64 - ref, vg)
        worst = sc.merge_max(worst, floor)
        got = sc.group_max((ref - plans[b].astype(np.longdouble))[free], vg[free])
        for k, v in got.items():
            assert v <= sc.GATE_FACTOR * floor[k], (k, v, floor[k])
        assert np.array_equal(ref[mask], plans[b][mask])
        far = sp.shift_warm(L, plans[b], 1e9, mask, plans[b], line, np.longdouble)
        assert not sp.shifted_mask(L, 1e9, mask).any()
        assert np.array_equal(far[free], line[free]) and np.array_equal(far[mask], plans[b][mask])
    print("shift_warm floor on the CPU [%s]: %s" % (name, worst))
    assert max(worst.values()) < 1e-9


def test_table_guess_on_the_grid_points_is_the_table_shifted_to_the_start():
    """At a grid point, with the table's own start, the interpolation returns that plan's free variables; a start moved by
    (a, b, c) moves every position variable of CoM and feet with it and nothing else."""
    cfg, O, L = sc.case("walk")
    rng = np.random.default_rng(5)
    dx, dy = np.array([0.2, 0.5, 0.9]), np.array([-0.1, 0.1])
    nodes = rng.normal(size=(2, 3, L.n_vars))
    start = np.zeros(24)
    for j in range(2):
        for i in range(3):
            ref = nodes[j, i]
            for s in range(6):
                start[3 * s:3 * s + 3] = ref[([L.off_lin, L.off_ang] + L.off_eem)[s]:][:3]
            goal = np.array([start[0] + dx[i], start[1] + dy[j], 0.24])
            free = ~sp.fixed_values(L, start, goal)[0]
            got = sp.table_guess(dx, dy, nodes, start, goal, L)
            # (goal - start is a float64 difference: the weight is 0 or 1 to rounding)
            assert np.abs(got - ref)[free].max() < 1e-13
            moved = start.copy()
            moved[0:3] += [0.3, -0.2, 0.01]
            moved[6:18] += np.tile([0.3, -0.2, 0.01], 4)
            got2 = sp.table_guess(dx, dy, nodes, moved, goal + [0.3, -0.2, 0.0], L)
            pos = free & (L.var_is_vel == 0) & ((L.var_set == 0) | ((L.var_set >= 2) & (L.var_set < 6)))
            assert np.abs((got2 - got)[pos] - np.array([0.3, -0.2, 0.01])[L.var_dim[pos]]).max() < 1e-13
            assert np.abs((got2 - got)[free & ~pos]).max() < 1e-13
    # outside the grid the weights are clamped; a 1 x 1 table has weight 0
    assert sp.table_cell(dx, dy, [0, 0], [5.0, -3.0])[4:] == (1.0, 0.0) and sp.table_cell(dx, dy, [0, 0], [-5.0, 3.0])[4:] == (0.0, 1.0)
    assert sp.table_cell(dx, dy, [0, 0], [5.0, 0.0])[:2] == (1, 2) and sp.table_cell(dx[:1], dy[:1], [0, 0], [5.0, 3.0]) == (0, 0, 0, 0, 0.0, 0.0)
