"""Shared by test_terrain_cpu.py and test_gpu_terrain.py: the probe table the terrain look-up (terrain_at in csrc/kernels.hpp and
its host copies) is held to oracle/terrain.py on, the evaluation points that put the feet of the smallest transcription on
those probes, what the statement expects of the terrain and force rows there, the gates and the accuracy record.  No tests in
here.

Dyadic grids.  cell = 2^-4, x0 = -0.25, y0 = -0.125, heights seeded integer multiples of 2^-10 below 2^-4 in magnitude, every
probe coordinate x0 + cell k / 4 with an integer k (or a far value, which is clamped before any arithmetic).  Then u and v of
the bilinear rule have two fractional bits, the heights ten, every product at most fourteen below a magnitude of 2^-4, every
sum is short and the divisions are by powers of two: every intermediate of h, hx, hy, hxy and of a terrain row z - h with a
dyadic z (ten fractional bits, |z| < 1) is exact in float64, in whatever order and however contracted.  These are compared
with ==.  What goes through a square root or a division by a norm (the force rows and their entries, on any grid) and
everything on the product's own grid (cell 1 / 110) is gated by measurement: GATE_FACTOR x the distance of the float64
statement from its longdouble form on the same probes, capped at the project's GATE_VALUE (values) and GATE_ENTRY_BILINEAR
(entries).

Probe classes, per axis (fx = grid coordinate, m = n - 1 the last node):
  node             0 < fx < m integral                    first_border   fx = 0
  interior         inside a cell but the last             last_border    fx = m
  last_cell        m - 1 < fx < m                         beyond_half    fx = -1/2, m + 1/2      (lo / hi)
  tie              fx = k + 1/2: where the nearest        beyond_two     fx = -2, m + 2
                   cell changes                           beyond_1e6     fx = -10^6, m + 10^6
  far_3e9, far_1e12  |fx| beyond int                      far_1e19       |fx| beyond int64
The table crosses every class of x with every class of y ("x:node,y:interior" is a probe on a grid line, "x:node,y:node" one
on a node, "x:interior,y:interior" one inside a cell), one probe per pair; a class a grid has no point of (a single row has
no interior) is absent from that grid's table.

sweep_plans() are the plans k_plan_check and k_force_fit sample the look-up with: the feet's x nodes ramp across the 5 x 7 grid
from beyond one border to beyond the other, one foot runs along a border line in y and one outside it (SWEEP_X, SWEEP_Y);
axis_class() names the class a sampled coordinate falls in."""
import itertools
import json
import os

import numpy as np

from conftest import ROOT  # noqa: F401  (path set-up)

import linearisation_cases as lc
from oracle import terrain as ot

CELL, X0, Y0 = 2.0 ** -4, -0.25, -0.125
HEIGHT_UNIT, HEIGHT_STEPS = 2.0 ** -10, 64                 # heights k 2^-10, |k| < 64
Z_UNIT = 2.0 ** -10
SHAPES = {"5x7": (5, 7), "2x2": (2, 2), "1x4": (1, 4), "4x1": (4, 1), "1x1": (1, 1)}
STACK_SHAPE, STACK_SEEDS = (5, 7), (11, 12, 13)
AXIS_CLASSES = ("node", "interior", "last_cell", "tie", "first_border", "last_border",
                "beyond_half_lo", "beyond_half_hi", "beyond_two_lo", "beyond_two_hi", "beyond_1e6_lo", "beyond_1e6_hi",
                "far_3e9_lo", "far_3e9_hi", "far_1e12_lo", "far_1e12_hi", "far_1e19_lo", "far_1e19_hi")
FAR_CLASSES = tuple(c for c in AXIS_CLASSES if c.startswith("far_"))
CASE = "two_base_polys"                                    # the smallest transcription of linearisation_cases
MAX_BATCH = 32
NEAR_LINE = 1e-9                                           # cells: a rounded fx this close to a line or a tie decides nothing
EXP5_SEED, EXP5_PROBES, EXP5_LEFT_OUT = 5, 256, 0          # test_terrain_cpu.py holds the count left out to this figure
MAX_LEFT_OUT = 0.01
STACK_MAP_ID = (2, 0, 1, -1, 3, 1, 0, 2, 3, -1)            # -1 and 3 = n_maps: terrain_at clamps them to the first and last map


def dyadic_grid(shape, seed):
    """Seeded heights k 2^-10, |k| < 64, no two neighbours equal (a flat cell would hide a wrong index)."""
    rng = np.random.default_rng(seed)
    while True:
        k = rng.integers(-HEIGHT_STEPS + 1, HEIGHT_STEPS, shape)
        if (shape[0] < 2 or (np.diff(k, axis=0) != 0).all()) and (shape[1] < 2 or (np.diff(k, axis=1) != 0).all()):
            return k * HEIGHT_UNIT


def grid(name):
    return dyadic_grid(SHAPES[name], 100 + list(SHAPES).index(name))


def stack():
    """Three different maps on one 5 x 7 grid."""
    return np.stack([dyadic_grid(STACK_SHAPE, s) for s in STACK_SEEDS])


def axis_probes(n):
    """class -> the grid coordinates fx of that class on an axis of n nodes (quarters of a cell, or far)."""
    m = n - 1
    quarters = [k / 4.0 for k in range(1, 4 * m)]
    out = {
        "node": [float(k) for k in range(1, m)],
        "interior": [f for f in quarters if f < m - 1 and (4 * f) % 2 == 1],
        "last_cell": [f for f in quarters if f > m - 1 and (4 * f) % 2 == 1],
        "tie": [k + 0.5 for k in range(m)],
        "first_border": [0.0], "last_border": [float(m)],
        "beyond_half_lo": [-0.5], "beyond_half_hi": [m + 0.5],
        "beyond_two_lo": [-2.0], "beyond_two_hi": [m + 2.0],
        "beyond_1e6_lo": [-1e6], "beyond_1e6_hi": [m + 1e6],
        "far_3e9_lo": [-3e9], "far_3e9_hi": [3e9], "far_1e12_lo": [-1e12], "far_1e12_hi": [1e12],
        "far_1e19_lo": [-1e19], "far_1e19_hi": [1e19],
    }
    return {c: out[c] for c in AXIS_CLASSES if out[c]}


class Probes:
    """names [n] ("x:<class>,y:<class>"), cx, cy [n] the two classes, x, y [n] float64."""

    def __init__(self, cx, cy, x, y):
        self.cx, self.cy = list(cx), list(cy)
        self.names = ["x:%s,y:%s" % c for c in zip(self.cx, self.cy)]
        self.x, self.y = np.asarray(x, np.float64), np.asarray(y, np.float64)

    def __len__(self):
        return len(self.names)


def table(shape):
    """The crossed probe table of a dyadic grid of this shape: one probe per pair of axis classes, the members of a class
    taken in turn."""
    ax, ay = axis_probes(shape[0]), axis_probes(shape[1])
    turn_x, turn_y = {c: itertools.cycle(v) for c, v in ax.items()}, {c: itertools.cycle(v) for c, v in ay.items()}
    cx, cy, x, y = [], [], [], []
    for a, b in itertools.product(ax, ay):
        cx.append(a), cy.append(b)
        x.append(X0 + CELL * next(turn_x[a])), y.append(Y0 + CELL * next(turn_y[b]))
    return Probes(cx, cy, x, y)


def is_far(probes):
    return np.array([a in FAR_CLASSES or b in FAR_CLASSES for a, b in zip(probes.cx, probes.cy)])


def exp5():
    """(H, cell, x0, y0) of the product's grid."""
    from qtos_amd import workloads
    H, cell = workloads.exp5_terrain()
    return np.asarray(H, np.float64), float(cell), -1.0, -1.0


def near_line(fx, n, what="both"):
    """Whether a grid coordinate is within NEAR_LINE cells of a grid line or border (what = "lines": where the bilinear slopes
    jump), of a nearest-cell tie (what = "ties": where the nearest cell's height jumps) or of either, on an axis of n nodes.
    Beyond the border by more than that nothing is decided."""
    f = np.asarray(fx, np.longdouble)
    lines = (f > -0.5) & (f < n - 0.5) & (np.abs(f - np.round(f)) < NEAR_LINE)
    ties = (f > 0) & (f < n - 1) & (np.abs(f - 0.5 - np.round(f - 0.5)) < NEAR_LINE)
    return {"lines": lines, "ties": ties, "both": lines | ties}[what]


def axis_class(fx, n):
    """The class (AXIS_CLASSES) of every grid coordinate fx on an axis of n nodes; a coordinate within NEAR_LINE cells of a node,
    border or tie counts as on it.  beyond_half: less than two cells beyond a border, beyond_two: two or more, beyond_1e6: 10^6
    or more, far_*: 3 10^9, 10^12, 10^19 or more."""
    m, out = n - 1, []
    for f in np.asarray(fx, np.float64).reshape(-1):
        side = "_lo" if f < 0 else "_hi"
        d = -f if f < 0 else f - m
        on_line, on_tie = abs(f - round(f)) < NEAR_LINE, abs(f - 0.5 - round(f - 0.5)) < NEAR_LINE
        if abs(f) < NEAR_LINE:
            out.append("first_border")
        elif abs(f - m) < NEAR_LINE:
            out.append("last_border")
        elif d > 0:
            name = ([c for c, lim in (("far_1e19", 1e19), ("far_1e12", 1e12), ("far_3e9", 3e9)) if abs(f) >= lim]
                    + [c for c, lim in (("beyond_1e6", 1e6), ("beyond_two", 2.0), ("beyond_half", 0.0)) if d >= lim])[0]
            out.append(name + side)
        else:
            out.append("node" if on_line else "tie" if on_tie else "last_cell" if f > m - 1 else "interior")
    return out


def exp5_probes(seed=EXP5_SEED, n=EXP5_PROBES):
    """Seeded probes on the product's grid: half over the ledges (x 0.3 .. 1.5, |y| < 0.3), the rest within three cells on
    either side of each of the four borders.  Returns (Probes, kept [n] bool): kept leaves out what near_line names."""
    H, cell, x0, y0 = exp5()
    nx, ny = H.shape
    rng = np.random.default_rng(seed)
    x1, y1 = x0 + (nx - 1) * cell, y0 + (ny - 1) * cell
    k = n // 8
    xs = [rng.uniform(0.3, 1.5, n - 4 * k)]
    ys = [rng.uniform(-0.3, 0.3, n - 4 * k)]
    names = ["ledges"] * (n - 4 * k)
    for name, bx, by in (("x_first", x0, None), ("x_last", x1, None), ("y_first", None, y0), ("y_last", None, y1)):
        xs.append(rng.uniform(bx - 3 * cell, bx + 3 * cell, k) if bx is not None else rng.uniform(x0 - 3 * cell, x1 + 3 * cell, k))
        ys.append(rng.uniform(by - 3 * cell, by + 3 * cell, k) if by is not None else rng.uniform(y0 - 3 * cell, y1 + 3 * cell, k))
        names += [name] * k
    P = Probes(names, names, np.concatenate(xs), np.concatenate(ys))
    kept = ~(near_line(ot.grid_coordinate(P.x, x0, cell), nx) | near_line(ot.grid_coordinate(P.y, y0, cell), ny))
    return P, kept


# ---- a plan whose feet sweep across the map (k_plan_check and k_force_fit as samplers of the look-up) -----------------------------

SWEEP_HZ, SWEEP_ROWS, SWEEP_WINDOWS, SWEEP_MAP_ID = 500.0, 600, 3, (2, 0, 1)
# grid coordinate of a foot's k-th position node (k = 0 .. 8; the even ones are its five stances, the odd ones its swings' mid
# nodes): start + k step.  The stances stand on beyond_two, beyond_half, node, interior, first_border and last_border, none
# on a nearest-cell tie (a whole stance would be undecided there); the swings cross every line and tie in between.
SWEEP_X = ((-3.0, 1.25), (-2.75, 1.25), (-3.0, 1.5), (-2.0, 1.5))
SWEEP_Y = (0.0, -1.5, 5.25, 2.25)                         # along the first border line, outside it, inside (twice)
SWEEP_CLASSES_X = {"node", "interior", "last_cell", "first_border", "last_border", "beyond_half_lo", "beyond_half_hi",
                   "beyond_two_lo", "beyond_two_hi"}
SWEEP_CLASSES_Y = {"first_border", "beyond_half_lo", "last_cell", "interior"}


def sweep_plans(seed=41, name=CASE):
    """SWEEP_WINDOWS random plans as spline_cases.random_plans makes them (need not be feasible) whose feet's x nodes are the
    ramps of SWEEP_X over the dyadic 5 x 7 grid and whose y stays at SWEEP_Y (y velocities zero).  Returns (plans, L)."""
    import spline_cases as sc
    cfg, O, L = lc.case(name)
    assert sc.TRANSCRIPTIONS[name]().phase_durations == cfg.phase_durations
    plans, _, _ = sc.random_plans(name, SWEEP_WINDOWS, seed)
    for e in range(4):
        S = L.splines[2 + e]
        k = 0
        for node in range(S.n_polys + 1):
            vx, vy = S.idx[node, 0, 0], S.idx[node, 0, 1]
            if node and vx == S.idx[node - 1, 0, 0]:
                continue                                   # the second node of a stance
            plans[:, vx] = X0 + CELL * (SWEEP_X[e][0] + k * SWEEP_X[e][1])
            plans[:, vy] = Y0 + CELL * SWEEP_Y[e]
            if S.idx[node, 1, 1] >= 0:
                plans[:, S.idx[node, 1, 1]] = 0.0
            k += 1
        assert k == 9
    return plans, L


def check_force_excess(fg, f, stance, f_max, dtype):
    """Columns 23 .. 26 of the plan check from the five force rows fg [n, 5] of a foot, its force f [n, 3] and its stance flag:
    in stance the largest excess over the rows' bounds, in swing the largest |component|."""
    fg, f = np.asarray(fg, dtype), np.asarray(f, dtype)
    ex = np.maximum.reduce([-fg[:, 0], fg[:, 0] - dtype(np.float64(f_max)), fg[:, 1], -fg[:, 2], fg[:, 3], -fg[:, 4]])
    return np.where(stance, ex, np.abs(f).max(axis=1))


# ---- the smallest transcription's rows that meet the terrain ---------------------------------------------------------------

def slots(L):
    """(stance [k, 3], swing [k, 3]): the (x, y, z) variables of the free stance footholds and of the free swing mid nodes."""
    stance, swing = [], []
    for e in range(4):
        S = L.splines[2 + e]
        for node in range(S.n_polys + 1):
            v = S.idx[node, 0]
            if L.fix_src[v[0]] >= 0 or any(tuple(v) == tuple(s) for s in stance + swing):
                continue
            (swing if S.idx[node, 1, 0] >= 0 else stance).append(tuple(int(a) for a in v))
    return np.array(stance), np.array(swing)


def terrain_rows(O, L):
    """[(row, vx, vy, vz)]: a terrain row per node 1 .. n_polys of every foot's motion spline."""
    out = []
    for e in range(4):
        S = L.splines[2 + e]
        out += [(O.L.off_terrain[e] + node - 1,) + tuple(int(a) for a in S.idx[node, 0]) for node in range(1, S.n_polys + 1)]
    return out


def force_instances(O, L, cfg):
    """[(row0, vsx, vsy, (vf0, vf1, vf2))]: five force rows per optimised node of every foot's force spline, with the x and y
    of the foothold of the stance the node lies in."""
    out, fpp = [], int(cfg.force_polys_per_stance)
    for e in range(4):
        F, S = L.splines[6 + e], L.splines[2 + e]
        node0, j = 0, 0
        for ph in range(len(cfg.phase_durations[e])):
            if ph % 2:
                node0 += 1
                continue
            foothold = S.idx[3 * (ph // 2), 0]
            for node in range(node0, node0 + fpp + 1):
                if F.idx[node, 0, 0] >= 0:
                    out.append((O.L.off_force[e] + 5 * j, int(foothold[0]), int(foothold[1]), tuple(int(a) for a in F.idx[node, 0])))
                    j += 1
            node0 += fpp
    return out


def eval_points(probes, seed=31, name=CASE):
    """Evaluation points like linearisation_cases.points with the free feet on the probes: the free stance footholds take the
    table in order, problem after problem, as many problems as the table needs; the free swing mid nodes take it in order as
    well (from the table's start, wrapping).  z of both is a seeded dyadic value.  Returns (x [B, n_vars], start, goal,
    at [B, n_vars] int: the probe a variable's foot stands on, -1 elsewhere)."""
    cfg, O, L = lc.case(name)
    stance, swing = slots(L)
    n = len(probes)
    B = -(-n // len(stance))
    assert B <= MAX_BATCH
    x, start, goal = lc.points(name, B, seed)
    rng = np.random.default_rng(seed + 1)
    at = np.full(x.shape, -1)
    for b in range(B):
        for group in (stance, swing):
            for s, (vx, vy, vz) in enumerate(group):
                k = (b * len(group) + s) % n
                x[b, vx], x[b, vy] = probes.x[k], probes.y[k]
                x[b, vz] = rng.integers(-1023, 1024) * Z_UNIT
                at[b, [vx, vy, vz]] = k
    return x, start, goal, at


def coverage(probes, at, name=CASE):
    """(classes met by a terrain row, classes met by a force instance) of the evaluation points' layout: sets of probe names."""
    cfg, O, L = lc.case(name)
    terr, force = set(), set()
    for b in range(len(at)):
        terr |= {probes.names[at[b, vx]] for _, vx, vy, vz in terrain_rows(O, L) if at[b, vx] >= 0}
        force |= {probes.names[at[b, vsx]] for _, vsx, vsy, _ in force_instances(O, L, cfg) if at[b, vsx] >= 0}
    return terr, force


def expected(x, H_of, mode, dtype, name=CASE):
    """What the statement expects of the rows that meet the terrain at the points x [B, n_vars]; H_of(b) = (H, cell, x0, y0) of
    problem b.  Returns a dict of arrays in dtype: terrain_rows [nt] / force_rows [nf] the row numbers, terrain_g [B, nt],
    terrain_J [B, nt, n_vars], force_g [B, nf], force_J [B, nf, n_vars] (whole rows of the node-space Jacobian), and
    terrain_var [nt] / force_var [nf]: the x variable of the foot a row stands on (eval_points' `at` names its probe)."""
    cfg, O, L = lc.case(name)
    tr, fi = terrain_rows(O, L), force_instances(O, L, cfg)
    B, nv = x.shape
    out = dict(terrain_rows=np.array([r[0] for r in tr]), force_rows=np.array([i[0] + k for i in fi for k in range(5)]),
               terrain_var=np.array([r[1] for r in tr]), force_var=np.array([i[1] for i in fi for k in range(5)]),
               terrain_g=np.empty((B, len(tr)), dtype), terrain_J=np.zeros((B, len(tr), nv), dtype),
               force_g=np.empty((B, 5 * len(fi)), dtype), force_J=np.zeros((B, 5 * len(fi), nv), dtype))
    vx, vy, vz = (np.array([r[k] for r in tr]) for k in (1, 2, 3))
    sx, sy = np.array([i[1] for i in fi]), np.array([i[2] for i in fi])
    vf = np.array([i[3] for i in fi])
    eye = np.eye(3)
    for b in range(B):
        H, cell, x0, y0 = H_of(b)
        h, hx, hy, _ = ot.lookup(H, cell, x0, y0, x[b, vx], x[b, vy], mode, dtype)
        out["terrain_g"][b] = x[b, vz].astype(dtype) - h
        k = np.arange(len(tr))
        out["terrain_J"][b, k, vx], out["terrain_J"][b, k, vy], out["terrain_J"][b, k, vz] = -hx, -hy, dtype(1)
        _, hx, hy, hxy = ot.lookup(H, cell, x0, y0, x[b, sx], x[b, sy], mode, dtype)
        val, ddx, ddy = ot.force_rows(x[b][vf], hx, hy, hxy, cfg.friction, dtype)
        out["force_g"][b] = val.reshape(-1)
        rows = (5 * np.arange(len(fi))[:, None] + np.arange(5)[None, :])
        out["force_J"][b, rows, sx[:, None]], out["force_J"][b, rows, sy[:, None]] = ddx, ddy
        for d in range(3):                                  # d row / d f_d: the row of the unit force along d
            unit = ot.force_rows(np.tile(eye[d], (len(fi), 1)), hx, hy, hxy, cfg.friction, dtype)[0]
            out["force_J"][b, rows, vf[:, d][:, None]] = unit
    return out


def masked(E, fx, row_kind):
    """expected()'s Jacobian rows as debug_eval hands them out: fixed columns and rows of kind 0 are zero."""
    E = dict(E)
    for k in ("terrain", "force"):
        J = E[k + "_J"].copy()
        J[:, :, fx] = 0
        J[:, row_kind[E[k + "_rows"]] == 0] = 0
        E[k + "_J"] = J
    return E


def gate(kind, floor):
    """GATE_FACTOR x the float64 statement's distance from its longdouble form on the same probes, capped at the project's
    gates: kind "value" (GATE_VALUE) or "entry" (GATE_ENTRY_BILINEAR)."""
    return min({"value": lc.GATE_VALUE, "entry": lc.GATE_ENTRY_BILINEAR}[kind], lc.GATE_FACTOR * float(floor))


def dist(a, b):
    """Largest absolute difference, in longdouble; nan where either has a non-finite entry the other has not."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    if not np.array_equal(np.isfinite(a), np.isfinite(b)):
        return float("nan")
    d = np.abs(a - b)[np.isfinite(a)]
    return float(d.max()) if d.size else 0.0


def record(section, name, entry):
    """Print a check's figures; where the environment variable QTOS_TERRAIN_ACCURACY names a file, keep them in it as JSON
    (profiles/terrain_accuracy.json is such a file from an MI355X run)."""
    print("terrain accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_TERRAIN_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
