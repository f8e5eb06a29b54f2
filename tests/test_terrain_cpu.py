"""The terrain look-up's index-free statement (oracle/terrain.py) held to itself, and every host copy of the rule held to the
statement on the whole probe table of terrain_cases.py: nodes, grid lines, borders, beyond the borders, far beyond them
(grid coordinates beyond int and int64), nearest-cell ties, single rows and columns, map ids outside the stack.  No GPU.

  the statement   its float64 and longdouble forms agree to the bit on the dyadic grids (what lets the other tests compare
                  with ==); Richardson quotients of h give hx, hy, hxy wherever the point is off the lines, outside the map
                  included (0 there); h is continuous across every line and border; on a line the slope is the right-hand
                  quotient (on the first border the rule's choice is the left-hand one: 0); force_rows' derivatives equal
                  Richardson quotients of its values
  the host copies plan_check.terrain_at, heightfield.height_at, feedback.terrain_lookup, Oracle.terrain_height and the terrain
                  and force rows of the oracle's constraints and jacobian: == on the dyadic grids where the quantity is exact,
                  within terrain_cases.gate elsewhere
  the oracle's Jacobian against Richardson quotients of its constraints at a point whose feet all lie beyond a border

Every test prints its figures (terrain_cases.record) before it asserts."""
import dataclasses

import numpy as np
import pytest

import linearisation_cases as lc
import terrain_cases as tc
from oracle import terrain as ot

LD = np.longdouble
MODES = pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "nearest"])
SHAPES = pytest.mark.parametrize("shape", list(tc.SHAPES))
OFF_LINE = ("interior", "last_cell", "tie") + tuple(c for c in tc.AXIS_CLASSES if c.startswith(("beyond", "far")))
OFF_TIE = ("node", "interior", "last_cell", "first_border", "last_border") + OFF_LINE[3:]
STEP = tc.CELL / 16                      # 2 STEP = cell / 8 < cell / 4, the probes' distance from the nearest line or tie


def _step(v, s):
    """A step a coordinate resolves: s, or four units in the last place of a far one."""
    return np.maximum(s, 4 * np.spacing(np.abs(v)))


def _lookup(H, P, mode, dtype=LD, dx=0.0, dy=0.0, grid=(tc.CELL, tc.X0, tc.Y0)):
    return ot.lookup(H, grid[0], grid[1], grid[2], P.x + dx, P.y + dy, mode, dtype)


def _oracle(mode, H, grid=(tc.CELL, tc.X0, tc.Y0)):
    from oracle.oracle import Oracle, oracle_dict
    cfg = dataclasses.replace(lc.case(tc.CASE)[0], terrain_mode=mode)
    return Oracle(oracle_dict(cfg), height=H, hcell=grid[0], hx0=grid[1], hy0=grid[2])


# ---- the table -----------------------------------------------------------------------------------------------------------

def test_the_table_has_every_class_and_every_crossing():
    P = tc.table(tc.SHAPES["5x7"])
    assert set(P.cx) == set(P.cy) == set(tc.AXIS_CLASSES)
    assert len(P) == len(tc.AXIS_CLASSES) ** 2 == len(set(P.names))
    # every coordinate is x0 + cell k / 4 or far
    for v, o in ((P.x, tc.X0), (P.y, tc.Y0)):
        f = (v - o) / tc.CELL
        assert np.all((np.abs(f) >= 3e9) | (4 * f == np.round(4 * f)))
    # a grid without interior points has no such class, a single node is both borders
    one = tc.axis_probes(1)
    assert "node" not in one and "interior" not in one and "tie" not in one and one["first_border"] == one["last_border"] == [0.0]
    assert set(tc.axis_probes(2)) == set(tc.AXIS_CLASSES) - {"node", "interior"}
    for name, shape in tc.SHAPES.items():
        H = tc.grid(name)
        assert H.shape == shape and np.abs(H).max() < 2.0 ** -4 and np.array_equal(H / tc.HEIGHT_UNIT, np.round(H / tc.HEIGHT_UNIT))
    S = tc.stack()
    assert S.shape == (3, 5, 7) and not any(np.array_equal(S[a], S[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_the_product_grid_probes_leave_out_at_most_one_percent():
    P, kept = tc.exp5_probes()
    left = int((~kept).sum())
    tc.record("cpu", "exp5_probes", dict(probes=len(P), left_out=left, share=left / len(P), seed=tc.EXP5_SEED))
    assert left == tc.EXP5_LEFT_OUT and left <= tc.MAX_LEFT_OUT * len(P)
    H, cell, x0, y0 = tc.exp5()
    # the ledges' probes do stand on different heights and all four borders have probes on either side
    h = ot.lookup(H, cell, x0, y0, P.x, P.y, 0)[0]
    assert len(np.unique(np.round(h[np.array(P.cx) == "ledges"].astype(float), 3))) > 3
    fx, fy = ot.grid_coordinate(P.x, x0, cell), ot.grid_coordinate(P.y, y0, cell)
    for f, n in ((fx, H.shape[0]), (fy, H.shape[1])):
        assert (f < 0).any() and ((f > 0) & (f < 3)).any() and (f > n - 1).any() and ((f < n - 1) & (f > n - 4)).any()


def test_the_sweep_plans_stances_stand_on_the_classes_they_name_and_on_no_tie():
    plans, L = tc.sweep_plans()
    nx, ny = tc.STACK_SHAPE
    stances, mids, ys = set(), set(), set()
    for e in range(4):
        S = L.splines[2 + e]
        for node in range(S.n_polys + 1):
            cls = tc.axis_class([(plans[0, S.idx[node, 0, 0]] - tc.X0) / tc.CELL], nx)[0]
            (mids if S.idx[node, 1, 0] >= 0 else stances).add(cls)
            ys.add(tc.axis_class([(plans[0, S.idx[node, 0, 1]] - tc.Y0) / tc.CELL], ny)[0])
            assert S.idx[node, 1, 1] < 0 or (plans[:, S.idx[node, 1, 1]] == 0).all()
    assert "tie" not in stances and "tie" in mids and "tie" not in ys
    assert stances >= tc.SWEEP_CLASSES_X - {"last_cell"} and ys == tc.SWEEP_CLASSES_Y
    assert len(plans) == tc.SWEEP_WINDOWS == len(tc.SWEEP_MAP_ID) and not np.array_equal(plans[0], plans[1])
    assert tc.axis_class([-3.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.25, 4.0, 4.5, 6.0, 1e6 + 4, 3e9, -1e19], nx) == [
        "beyond_two_lo", "beyond_half_lo", "first_border", "interior", "tie", "node", "last_cell", "last_border", "beyond_half_hi",
        "beyond_two_hi", "beyond_1e6_hi", "far_3e9_hi", "far_1e19_lo"]


# ---- the statement against itself ----------------------------------------------------------------------------------------

@SHAPES
@MODES
def test_float64_and_longdouble_statement_agree_to_the_bit_on_the_dyadic_grids(shape, mode):
    H, P = tc.grid(shape), tc.table(tc.SHAPES[shape])
    a, b = _lookup(H, P, mode, np.float64), _lookup(H, P, mode, LD)
    for u, v in zip(a, b):
        assert u.dtype == np.float64 and v.dtype == LD and np.array_equal(u.astype(LD), v)
    # and a terrain row with a dyadic z
    z = np.random.default_rng(1).integers(-1023, 1024, len(P)) * tc.Z_UNIT
    assert np.array_equal((z - a[0]).astype(LD), z.astype(LD) - b[0])


def test_non_finite_coordinates_have_no_terrain():
    H = tc.grid("5x7")
    for mode in (0, 1):
        out = ot.lookup(H, tc.CELL, tc.X0, tc.Y0, [0.0, np.nan, np.inf, 0.0], [0.0, 0.0, 0.0, -np.inf], mode)
        for a in out:
            assert np.array_equal(np.isnan(a), [False, True, True, True])


def _richardson(fun, s):
    """R(s) and R(s / 2) of the central difference quotients fun(step)."""
    d1, d2, d4 = fun(s), fun(s / 2), fun(s / 4)
    return (4 * d2 - d1) / 3, (4 * d4 - d2) / 3


@pytest.mark.parametrize("grid", ["5x7", "2x2", "1x4", "4x1", "exp5"])
@MODES
def test_richardson_quotients_of_h_give_the_slopes_off_the_lines_and_outside_the_map(grid, mode):
    if grid == "exp5":
        H, cell, x0, y0 = tc.exp5()
        P, kept = tc.exp5_probes()
        s = lc.FD_STEP_TERRAIN
        fx, fy = ot.grid_coordinate(P.x, x0, cell), ot.grid_coordinate(P.y, y0, cell)
        half = 0.5 * mode                                 # the kinks: the lines (bilinear), the ties (nearest)
        okx = np.abs(fx - half - np.round(fx - half)) * cell > 2 * s
        oky = np.abs(fy - half - np.round(fy - half)) * cell > 2 * s
        okx, oky = okx | (fx < -0.5) | (fx > H.shape[0] - 0.5), oky | (fy < -0.5) | (fy > H.shape[1] - 0.5)
    else:
        H, (cell, x0, y0) = tc.grid(grid), (tc.CELL, tc.X0, tc.Y0)
        P, s = tc.table(tc.SHAPES[grid]), STEP
        ok = OFF_TIE if mode == 1 else OFF_LINE
        okx, oky = np.array([c in ok for c in P.cx]), np.array([c in ok for c in P.cy])
    g = (cell, x0, y0)
    sx, sy = _step(P.x, s), _step(P.y, s)

    def h(dx, dy):
        return _lookup(H, P, mode, LD, dx, dy, g)[0]

    def span(v, d):                                       # the step the two arguments really differ by
        return (v + d).astype(LD) - (v - d).astype(LD)
    qx = _richardson(lambda k: (h(sx * k / s, 0) - h(-sx * k / s, 0)) / span(P.x, sx * k / s), s)
    qy = _richardson(lambda k: (h(0, sy * k / s) - h(0, -sy * k / s)) / span(P.y, sy * k / s), s)
    qxy = _richardson(lambda k: (h(sx * k / s, sy * k / s) - h(sx * k / s, -sy * k / s) - h(-sx * k / s, sy * k / s)
                                 + h(-sx * k / s, -sy * k / s)) / (span(P.x, sx * k / s) * span(P.y, sy * k / s)), s)
    _, hx, hy, hxy = _lookup(H, P, mode, LD, grid=g)
    entry = dict(probes=len(P), step=s)
    for what, q, ref, ok_ in (("hx", qx, hx, okx), ("hy", qy, hy, oky), ("hxy", qxy, hxy, okx & oky)):
        assert ok_.sum() > (0 if grid in ("1x4", "4x1") else len(P) // 3)
        floor = float(np.abs(q[0] - q[1])[ok_].max()) if ok_.any() else 0.0
        entry[what] = dict(probes=int(ok_.sum()), floor=floor, gate=lc.GATE_FACTOR * floor,
                           achieved=float(np.abs(ref - q[0])[ok_].max()) if ok_.any() else 0.0,
                           largest=float(np.abs(ref[ok_]).max()) if ok_.any() else 0.0)
    tc.record("cpu_richardson_" + ("nearest" if mode else "bilinear"), grid, entry)
    for what in ("hx", "hy", "hxy"):
        assert entry[what]["achieved"] <= entry[what]["gate"], (what, entry[what])
    if mode == 0 and grid in ("5x7", "exp5"):
        assert entry["hx"]["largest"] > 0.5 and entry["hy"]["largest"] > 0.5
        assert grid == "exp5" or entry["hxy"]["largest"] > 0.5     # (the ledges of exp_5 are steps along one axis: hxy = 0 but at corners)
        outside = np.array([c.startswith(("beyond", "far")) for c in P.cx]) if grid == "5x7" else (fx < 0) | (fx > H.shape[0] - 1)
        assert outside.any() and np.all(hx[outside] == 0) and np.all(qx[0][outside & okx] == 0) and np.all(hxy[outside] == 0)


@pytest.mark.parametrize("grid", ["5x7", "2x2", "1x4", "4x1", "1x1"])
def test_h_is_continuous_across_every_line_and_border_and_the_slope_on_a_line_is_the_right_hand_quotient(grid):
    H, P = tc.grid(grid), tc.table(tc.SHAPES[grid])
    h, hx, hy, _ = _lookup(H, P, 0)
    d = tc.CELL * 2.0 ** -20
    # |h(x + d) - h(x)| <= d x the steepest slope of any cell edge (+ the mixed term, of a smaller order)
    steep = max([np.abs(np.diff(H, axis=a)).max() for a in (0, 1) if H.shape[a] > 1] + [0.0]) / tc.CELL
    worst = 0.0
    for dx, dy in ((d, 0), (-d, 0), (0, d), (0, -d), (d, d), (-d, -d)):
        near = ~tc.is_far(P)
        worst = max(worst, float(np.abs(_lookup(H, P, 0, LD, dx, dy)[0] - h)[near].max()))
    tc.record("cpu_continuity", grid, dict(step=d, bound=4 * d * steep, achieved=worst))
    assert worst <= 4 * d * steep
    # on a line: the right-hand quotient (exact: the surface is linear along an axis inside a cell); at and beyond the last
    # border that is 0.  On the first border the rule returns the left-hand one, 0 -- a point on the border counts as clamped.
    s = STEP
    for cls, slope, q in ((P.cx, hx, (_lookup(H, P, 0, LD, s, 0)[0] - h) / LD(s)), (P.cy, hy, (_lookup(H, P, 0, LD, 0, s)[0] - h) / LD(s))):
        cls = np.array(cls)
        on = (cls == "node") | (cls == "last_border")
        assert np.array_equal(slope[on], q[on])
        first = cls == "first_border"
        assert np.all(slope[first] == 0)
        if grid == "5x7":
            assert (cls == "node").sum() > 10 and np.abs(q[cls == "node"]).max() > 0.5 and np.abs(q[first]).max() > 0.5


def test_force_row_derivatives_equal_richardson_quotients_of_the_values():
    cfg = lc.case(tc.CASE)[0]
    H, P = tc.grid("5x7"), tc.table(tc.SHAPES["5x7"])
    inside = np.array([a in ("interior", "last_cell", "tie") and b in ("interior", "last_cell", "tie") for a, b in zip(P.cx, P.cy)])
    P = tc.Probes(np.array(P.cx)[inside], np.array(P.cy)[inside], P.x[inside], P.y[inside])
    f = np.random.default_rng(3).normal(size=(len(P), 3)) * lc.NOISE_FORCE
    s = tc.CELL * 2.0 ** -12

    def val(dx, dy):
        return ot.force_rows(f, *_lookup(H, P, 0, LD, dx, dy)[1:], cfg.friction)[0]
    qx = _richardson(lambda k: (val(k, 0) - val(-k, 0)) / ((P.x + k).astype(LD) - (P.x - k).astype(LD))[:, None], s)
    qy = _richardson(lambda k: (val(0, k) - val(0, -k)) / ((P.y + k).astype(LD) - (P.y - k).astype(LD))[:, None], s)
    _, ddx, ddy = ot.force_rows(f, *_lookup(H, P, 0)[1:], cfg.friction)
    floor = float(max(np.abs(qx[0] - qx[1]).max(), np.abs(qy[0] - qy[1]).max()))
    achieved = float(max(np.abs(ddx - qx[0]).max(), np.abs(ddy - qy[0]).max()))
    tc.record("cpu_richardson_force_rows", "5x7", dict(probes=len(P), step=s, floor=floor, gate=lc.GATE_FACTOR * floor,
                                                       achieved=achieved, largest=float(np.abs(ddx).max())))
    assert len(P) == 9 and np.abs(ddx).max() > 1.0 and np.abs(ddy).max() > 1.0      # hxy does enter
    assert achieved <= lc.GATE_FACTOR * floor


# ---- the host copies against the statement -----------------------------------------------------------------------------------

def _same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


@SHAPES
@MODES
def test_host_look_ups_equal_the_statement_on_the_dyadic_table(shape, mode):
    from qtos_amd import feedback, heightfield, plan_check
    H, P = tc.grid(shape), tc.table(tc.SHAPES[shape])
    h, hx, hy, _ = _lookup(H, P, mode, np.float64)
    far = tc.is_far(P)
    wrong = {}
    got = plan_check.terrain_at((H, tc.CELL, tc.X0, tc.Y0), mode, P.x, P.y, np.float64)
    got_ld = plan_check.terrain_at((H, tc.CELL, tc.X0, tc.Y0), mode, P.x, P.y, LD)
    for k, ref in enumerate((h, hx, hy)):
        wrong["plan_check.terrain_at[%d]" % k] = (got[k] != ref) | (got_ld[k] != ref)
    wrong["heightfield.height_at"] = heightfield.height_at(H, tc.CELL, P.x, P.y, tc.X0, tc.Y0, mode) != h
    look = feedback.terrain_lookup(H, tc.CELL, tc.X0, tc.Y0, mode)
    wrong["feedback.terrain_lookup"] = np.array([look(0, a, b) for a, b in zip(P.x, P.y)]) != h
    O = _oracle(mode, H)
    wrong["Oracle.terrain_height"] = np.array([O.terrain_height(a, b) for a, b in zip(P.x, P.y)]) != h
    entry = {k: dict(wrong=int(v.sum()), wrong_far=int((v & far).sum()), first=(P.names[int(np.argmax(v))] if v.any() else None))
             for k, v in wrong.items()}
    tc.record("cpu_host_" + ("nearest" if mode else "bilinear"), shape, dict(probes=len(P), far=int(far.sum()), **entry))
    assert not any(v.any() for v in wrong.values()), entry


def test_feedback_terrain_lookup_clamps_the_map_id():
    from qtos_amd import feedback
    S, P = tc.stack(), tc.table(tc.STACK_SHAPE)
    for mode in (0, 1):
        look = feedback.terrain_lookup(S, tc.CELL, tc.X0, tc.Y0, mode)
        for mid, m in ((-1, 0), (0, 0), (1, 1), (2, 2), (3, 2), (7, 2), (-2 ** 31, 0)):
            h = ot.lookup(S[m], tc.CELL, tc.X0, tc.Y0, P.x, P.y, mode, np.float64)[0]
            assert _same([look(mid, a, b) for a, b in zip(P.x, P.y)], h), (mode, mid)


@MODES
def test_host_look_ups_are_within_the_measured_gate_on_the_product_grid(mode):
    from qtos_amd import heightfield, plan_check
    H, cell, x0, y0 = tc.exp5()
    P, kept = tc.exp5_probes()
    P = tc.Probes(np.array(P.cx)[kept], np.array(P.cy)[kept], P.x[kept], P.y[kept])
    ref, f64 = ot.lookup(H, cell, x0, y0, P.x, P.y, mode, LD), ot.lookup(H, cell, x0, y0, P.x, P.y, mode, np.float64)
    floors = [tc.dist(f64[k], ref[k]) for k in range(3)]
    gates = [tc.gate("value", floors[0]), tc.gate("entry", floors[1]), tc.gate("entry", floors[2])]
    got = plan_check.terrain_at((H, cell, x0, y0), mode, P.x, P.y, np.float64)
    O = _oracle(mode, H, (cell, x0, y0))
    achieved = {"plan_check.terrain_at[%d]" % k: tc.dist(got[k], ref[k]) for k in range(3)}
    achieved["heightfield.height_at"] = tc.dist(heightfield.height_at(H, cell, P.x, P.y, x0, y0, mode), ref[0])
    achieved["Oracle.terrain_height"] = tc.dist([O.terrain_height(a, b) for a, b in zip(P.x, P.y)], ref[0])
    tc.record("cpu_host_" + ("nearest" if mode else "bilinear"), "exp5", dict(probes=len(P), floors=floors, gates=gates, achieved=achieved))
    for k, v in achieved.items():
        assert v <= gates[int(k[-2]) if k.endswith("]") else 0], (k, v)


def _oracle_rows(mode, H_of, x, at, exact):
    """The oracle's terrain and force rows at the points x against the statement: where `exact`, the terrain rows of the feet
    that stand on probes (at >= 0; the fixed first stances keep their start values, which are not dyadic) with ==; all rows
    within the gate.  Returns the record's entry."""
    E, F = tc.expected(x, H_of, mode, LD), tc.expected(x, H_of, mode, np.float64)
    floor_v, floor_e = tc.dist(F["force_g"], E["force_g"]), tc.dist(F["force_J"], E["force_J"])
    floor_tv, floor_te = tc.dist(F["terrain_g"], E["terrain_g"]), tc.dist(F["terrain_J"], E["terrain_J"])
    entry = dict(problems=len(x), terrain_rows=len(E["terrain_rows"]), force_rows=len(E["force_rows"]),
                 floor=dict(terrain_values=floor_tv, terrain_entries=floor_te, force_values=floor_v, force_entries=floor_e),
                 gate=dict(terrain_values=tc.gate("value", floor_tv), terrain_entries=tc.gate("entry", floor_te),
                           force_values=tc.gate("value", floor_v), force_entries=tc.gate("entry", floor_e)))
    ach = dict(terrain_values=0.0, terrain_entries=0.0, force_values=0.0, force_entries=0.0)
    exact_ok = True
    on = at[:, E["terrain_var"]] >= 0                      # [B, nt]
    assert on.sum() > on.size // 2
    for b in range(len(x)):
        O = _oracle(mode, *_grid_args(H_of(b)))
        g, J = O.constraints(x[b]), O.jacobian(x[b])
        for k in ("terrain", "force"):
            ach[k + "_values"] = max(ach[k + "_values"], tc.dist(g[E[k + "_rows"]], E[k + "_g"][b]))
            ach[k + "_entries"] = max(ach[k + "_entries"], tc.dist(J[E[k + "_rows"]], E[k + "_J"][b]))
        r = E["terrain_rows"][on[b]]
        exact_ok &= _same(g[r], E["terrain_g"][b][on[b]]) and _same(J[r], E["terrain_J"][b][on[b]])
    entry["achieved"], entry["terrain_rows_equal"] = ach, bool(exact_ok)
    if exact:                                              # the float64 statement is exact there
        assert tc.dist(F["terrain_g"][on], E["terrain_g"][on]) == 0 and tc.dist(F["terrain_J"][on], E["terrain_J"][on]) == 0
    return entry


def _grid_args(g):
    return g[0], (g[1], g[2], g[3])


def _assert_rows(entry, exact):
    for k, v in entry["achieved"].items():
        assert v <= entry["gate"][k], (k, v, entry["gate"][k])
    if exact:
        assert entry["terrain_rows_equal"]


@SHAPES
@MODES
def test_oracle_terrain_and_force_rows_equal_the_statement_with_the_feet_on_the_table(shape, mode):
    H, P = tc.grid(shape), tc.table(tc.SHAPES[shape])
    x, _, _, at = tc.eval_points(P)
    terr, force = tc.coverage(P, at)
    assert terr == force == set(P.names)                  # every probe under a terrain row and under a force instance
    entry = _oracle_rows(mode, lambda b: (H, tc.CELL, tc.X0, tc.Y0), x, at, exact=True)
    tc.record("cpu_oracle_rows_" + ("nearest" if mode else "bilinear"), shape, entry)
    _assert_rows(entry, True)
    if mode == 0 and shape == "5x7":
        assert entry["floor"]["force_entries"] > 0        # hxy does enter somewhere


@MODES
def test_oracle_terrain_and_force_rows_are_within_the_measured_gate_on_the_product_grid(mode):
    H, cell, x0, y0 = tc.exp5()
    P, kept = tc.exp5_probes()
    P = tc.Probes(np.array(P.cx)[kept], np.array(P.cy)[kept], P.x[kept], P.y[kept])
    x, _, _, at = tc.eval_points(P)
    entry = _oracle_rows(mode, lambda b: (H, cell, x0, y0), x, at, exact=False)
    tc.record("cpu_oracle_rows_" + ("nearest" if mode else "bilinear"), "exp5", entry)
    _assert_rows(entry, False)


def test_oracle_jacobian_against_richardson_differences_beyond_the_border():
    """The region the seeds of test_linearisation_cpu.py never reach: every foot, the fixed first stances too, more than 2 h
    beyond a border in x or in y -- in one axis only for most, so that one slope is zero, the other is not and the mixed
    derivative must be zero."""
    cfg, _, L = lc.case(tc.CASE)
    H, P = tc.grid("5x7"), tc.table(tc.SHAPES["5x7"])
    O = _oracle(0, H)
    beyond = tuple(c for c in tc.AXIS_CLASSES if c.startswith("beyond_half") or c.startswith("beyond_two"))
    inside = ("interior", "last_cell", "tie")
    pick = [k for k in range(len(P)) if (P.cx[k] in beyond and P.cy[k] in inside + beyond) or (P.cy[k] in beyond and P.cx[k] in inside)]
    x, _, _ = lc.points(tc.CASE, 1, 9)
    x = x[0]
    feet = lc.foot_motion(L) & (L.var_is_vel == 0)
    vx, vy = np.nonzero(feet & (L.var_dim == 0))[0], np.nonzero(feet & (L.var_dim == 1))[0]
    assert len(vx) == len(vy) <= len(pick)
    pick = np.array(pick)[np.linspace(0, len(pick) - 1, len(vx)).astype(int)]
    x[vx], x[vy] = P.x[pick], P.y[pick]
    h = lc.FD_STEP_TERRAIN
    fx, fy = (x[vx] - tc.X0) / tc.CELL, (x[vy] - tc.Y0) / tc.CELL
    out = (fx < 0) | (fx > H.shape[0] - 1) | (fy < 0) | (fy > H.shape[1] - 1)
    assert out.all() and tc.CELL / 4 > 2 * h              # (the picked classes are a quarter cell or more from border and lines)
    slopes = ot.lookup(H, tc.CELL, tc.X0, tc.Y0, x[vx], x[vy], 0)
    assert (slopes[1] != 0).any() and (slopes[2] != 0).any() and np.all(slopes[3] == 0)
    cols = np.nonzero(L.var_set >= 2)[0]
    floor, gate, achieved = lc.fd_check(O, x, cols, h)
    tc.record("cpu_oracle_fd_beyond_border", tc.CASE, dict(columns=len(cols), h=h, feet=len(vx), floor=floor, gate=gate, achieved=achieved))
    assert achieved <= gate
