"""numpy restatement of the spline layer (TEST INFRASTRUCTURE, like everything under oracle/).

Three kernels of the product turn a node vector into numbers through the cubic-Hermite splines: k_sample (the CSV
rows), k_shift_warm (the time-shifted warm start of a replan) and the starting-point code (straight-line guess /
nominal-plan table, k_debug_guess and k_start).  This file states the layer they stand on once more, in numpy and
with the arithmetic's number type as a parameter, so that the tests need not take the product's word -- nor the C
oracle's -- for it:

  * layout(cfg)         the ten splines (lin, ang, four foot-motion, four foot-force) of a PlannerConfig: polynomial
                        durations, the (node, q, d) -> variable index, and per variable its descriptors
  * eval_spline(...)    one spline (or its first derivative) at given times
  * sample_rows(...)    the 37-column CSV rows
  * shift_warm(...)     the time-shifted warm start
  * table_guess(...)    the starting point interpolated from a table of nominal plans

Written from the layout documented in oracle/qtos_oracle.c (build_model, locate, hermite_w) and from PlannerConfig; it
does not call the oracle library.  dtype = np.longdouble is the reference the kernels are held to, dtype = np.float64
the same formulas in the kernels' own precision: the distance between the two is the rounding floor the tests derive
their gates from.

Variable layout (towr order): base splines off + 6 node + 3 q + d (q = 0 position / 1 velocity); a foot's motion
spline 3 variables per stance (x, y, z: shared by the two nodes of the stance) and 5 per swing (x, vx, y, vy, z of the
mid node); a foot's force spline 6 per node that touches no swing polynomial (x, dx, y, dy, z, dz).
"""
import numpy as np

NEE = 4
N_SETS = 2 + 2 * NEE
START_DOUBLES = 24
# fix_src of a variable: -1 free, 0 .. 23 that entry of the start vector, 24 / 25 goal x / y, 26 constant zero
FIX_GOAL, FIX_ZERO = 24, 26
LOCATE_EPS = 1e-10      # a time within this of a junction belongs to the polynomial in front of it
HORIZON_EPS = 1e-9      # a node within this behind the previous plan's horizon is still read from it (at the horizon)


class Spline:
    """dur [n_polys] float64, idx [n_polys + 1, 2, 3] int: variable of (node, q, d), -1 = constant zero."""

    def __init__(self, dur, idx):
        self.dur = np.asarray(dur, np.float64)
        self.idx = np.asarray(idx, np.int64).reshape(len(self.dur) + 1, 2, 3)
        self.n_polys = len(self.dur)

    def node_times(self):
        """Time of every node: the durations in front of it, summed one by one in float64 (as the product's tables are)."""
        return np.concatenate([[0.0], np.cumsum(self.dur)])


class Layout:
    pass


def _base_durations(T, dt):
    dur, t_left = [], T
    while t_left > 1e-10:
        dur.append(dt if t_left > dt else t_left)
        t_left -= dt
    return dur


def layout(cfg):
    """The spline layer of a PlannerConfig.  Attributes: splines (ten Spline: lin, ang, motion of feet 0 .. 3, force of
    feet 0 .. 3), T, n_base_nodes, n_vars, off_lin, off_ang, off_eem[4], off_eef[4], n_eem[4], n_eef[4] and per variable
    var_set (0 .. 9), var_node, var_is_vel, var_dim, node_time, fix_src.  Where two nodes share a variable (a stance's
    foothold) the later node's index and time are the variable's."""
    L = Layout()
    phases = [[float(d) for d in foot] for foot in cfg.phase_durations]
    T = 0.0
    for d in phases[0]:
        T += d
    L.T = T
    base = _base_durations(T, float(cfg.dt_base))
    nb = len(base)
    L.n_base_nodes = nb + 1
    L.off_lin, L.off_ang = 0, 6 * (nb + 1)
    splines = []
    for off in (L.off_lin, L.off_ang):
        idx = off + 6 * np.arange(nb + 1)[:, None, None] + 3 * np.arange(2)[None, :, None] + np.arange(3)[None, None, :]
        splines.append(Spline(base, idx))
    off = 12 * (nb + 1)
    L.off_eem, L.n_eem, L.off_eef, L.n_eef = [], [], [], []
    for e in range(NEE):                                  # foot motion: stance = one constant polynomial, swing = two
        P = len(phases[e])
        if P < 1 or P % 2 == 0:
            raise ValueError("a foot's schedule starts and ends with a stance")
        dur, idx, v = [], [[[-1] * 3, [-1] * 3]], off
        for ph, d in enumerate(phases[e]):
            if ph % 2 == 0:
                idx[-1] = [[v, v + 1, v + 2], [-1] * 3]
                idx.append([[v, v + 1, v + 2], [-1] * 3])
                dur.append(d)
                v += 3
            else:
                dur += [d / 2, d / 2]
                idx.append([[v, v + 2, v + 4], [v + 1, v + 3, -1]])
                idx.append([[-1] * 3, [-1] * 3])          # (start of the next stance: filled in by it)
                v += 5
        splines.append(Spline(dur, idx))
        L.off_eem.append(off)
        L.n_eem.append(v - off)
        off = v
    fpp = int(cfg.force_polys_per_stance)
    for e in range(NEE):                                  # foot force: fpp polynomials per stance, one zero polynomial per swing
        dur, swing = [], []
        for ph, d in enumerate(phases[e]):
            if ph % 2 == 0:
                dur += [d / fpp] * fpp
                swing += [False] * fpp
            else:
                dur.append(d)
                swing.append(True)
        idx, v = [], off
        for node in range(len(dur) + 1):
            if (node > 0 and swing[node - 1]) or (node < len(dur) and swing[node]):
                idx.append([[-1] * 3, [-1] * 3])
            else:
                idx.append([[v, v + 2, v + 4], [v + 1, v + 3, v + 5]])
                v += 6
        splines.append(Spline(dur, idx))
        L.off_eef.append(off)
        L.n_eef.append(v - off)
        off = v
    L.splines, L.n_vars = splines, off
    n = L.n_vars
    L.var_set, L.var_node = np.full(n, -1), np.full(n, -1)
    L.var_is_vel, L.var_dim = np.full(n, -1), np.full(n, -1)
    L.node_time = np.zeros(n)
    for s, S in enumerate(splines):
        nt = S.node_times()
        for node in range(S.n_polys + 1):                 # in node order: the later node sharing a variable wins
            for q in range(2):
                for d in range(3):
                    v = S.idx[node, q, d]
                    if v >= 0:
                        L.var_set[v], L.var_node[v], L.var_is_vel[v], L.var_dim[v], L.node_time[v] = s, node, q, d, nt[node]
    if (L.var_set < 0).any():
        raise AssertionError("a variable belongs to no spline")
    # fixed variables: start state, goal x / y, zero final velocity / attitude / rates; the start velocities where the
    # configuration honours them
    L.fix_src = np.full(n, -1)
    hv = bool(cfg.honor_start_velocity)
    for d in range(3):
        L.fix_src[L.off_lin + d] = d
        L.fix_src[L.off_lin + 3 + d] = 18 + d if hv else FIX_ZERO
        L.fix_src[L.off_ang + d] = 3 + d
        L.fix_src[L.off_ang + 3 + d] = 21 + d if hv else FIX_ZERO
        if d < 2:
            L.fix_src[L.off_lin + 6 * nb + d] = FIX_GOAL + d
        L.fix_src[L.off_lin + 6 * nb + 3 + d] = FIX_ZERO
        L.fix_src[L.off_ang + 6 * nb + d] = FIX_ZERO
        L.fix_src[L.off_ang + 6 * nb + 3 + d] = FIX_ZERO
        for e in range(NEE):
            L.fix_src[L.off_eem[e] + d] = 6 + 3 * e + d
    return L


def fixed_values(L, start, goal):
    """(mask, values) of the fixed variables of a problem, from the layout's descriptors."""
    src = np.concatenate([np.asarray(start, np.float64)[:START_DOUBLES], np.asarray(goal, np.float64)[:2], [0.0]])
    mask = L.fix_src >= 0
    val = np.zeros(L.n_vars)
    val[mask] = src[L.fix_src[mask]]
    return mask, val


def _hermite_w(T, t, deriv):
    """Weights of (p0, v0, p1, v1) of a cubic Hermite polynomial of duration T at local time t, value or first derivative."""
    T2 = T * T
    T3 = T2 * T
    t2 = t * t
    t3 = t2 * t
    if deriv == 0:
        return (1 - 3 * t2 / T2 + 2 * t3 / T3, t - 2 * t2 / T + t3 / T2, 3 * t2 / T2 - 2 * t3 / T3, -t2 / T + t3 / T2)
    if deriv == 1:
        return (-6 * t / T2 + 6 * t2 / T3, 1 - 4 * t / T + 3 * t2 / T2, 6 * t / T2 - 6 * t2 / T3, -2 * t / T + 3 * t2 / T2)
    raise ValueError("deriv is 0 or 1")


def eval_spline(L, s, x, t, deriv=0, dtype=np.longdouble):
    """Spline s (0 lin, 1 ang, 2 + e foot e's motion, 6 + e foot e's force) of the node vector x [n_vars] (or one node
    vector per time, [n, n_vars]) at the times t [n] (float64 data), value (deriv 0) or first derivative (deriv 1): [n, 3]
    in dtype.

    The polynomial of a time t is the FIRST one whose end is >= t - 1e-10: at a junction the polynomial in front of it;
    behind the last end the last one.  Its local time is t minus the durations in front of it, taken off one by one."""
    S = L.splines[s]
    t = np.atleast_1d(np.asarray(t, np.float64)).astype(dtype)
    x = np.asarray(x, np.float64).astype(dtype)
    dur = S.dur.astype(dtype)
    ends = np.cumsum(dur, dtype=dtype)
    k = np.minimum(np.searchsorted(ends, t - dtype(LOCATE_EPS), side="left"), S.n_polys - 1)
    tau = t.copy()
    for i in range(int(k.max()) if len(k) else 0):
        tau = np.where(k > i, tau - dur[i], tau)
    w = _hermite_w(dur[k], tau, deriv)
    out = np.zeros((len(t), 3), dtype)
    for d in range(3):
        acc = np.zeros(len(t), dtype)
        for a in range(4):
            var = S.idx[k + (a >> 1), a & 1, d]
            xv = x[np.maximum(var, 0)] if x.ndim == 1 else x[np.arange(len(t)), np.maximum(var, 0)]
            acc = acc + w[a] * np.where(var >= 0, xv, dtype(0))
        out[:, d] = acc
    return out


def sample_rows(L, x, t0, hz, n_rows, dtype=np.longdouble):
    """The CSV rows of a plan: column 0 the time stamp t0 + k / hz, then the state at plan time min(k / hz, T) -- CoM 1 .. 3,
    Euler 4 .. 6, feet 7 .. 18, CoM velocity 19 .. 21, Euler rates 22 .. 24, foot forces 25 .. 36.  k / hz is the float64
    quotient (it is data: the plan time the kernels evaluate at), everything behind it is dtype."""
    tk = np.arange(n_rows) / np.float64(hz)
    rows = np.zeros((n_rows, 37), dtype)
    rows[:, 0] = dtype(np.float64(t0)) + tk.astype(dtype)
    t = np.minimum(tk, L.T)
    rows[:, 1:4] = eval_spline(L, 0, x, t, 0, dtype)
    rows[:, 4:7] = eval_spline(L, 1, x, t, 0, dtype)
    for e in range(NEE):
        rows[:, 7 + 3 * e:10 + 3 * e] = eval_spline(L, 2 + e, x, t, 0, dtype)
        rows[:, 25 + 3 * e:28 + 3 * e] = eval_spline(L, 6 + e, x, t, 0, dtype)
    rows[:, 19:22] = eval_spline(L, 0, x, t, 1, dtype)
    rows[:, 22:25] = eval_spline(L, 1, x, t, 1, dtype)
    return rows


def shifted_mask(L, offset, fixed_mask):
    """The free variables a shift by `offset` still reads from the previous plan (the others get the straight line)."""
    return ~np.asarray(fixed_mask, bool) & (np.float64(offset) + L.node_time <= L.T + HORIZON_EPS)


def shift_warm(L, x_prev, offset, fixed_mask, fixed_values, straight_line, dtype=np.longdouble):
    """The time-shifted warm start of a replan, [n_vars] in dtype: fixed variables carry fixed_values; a free variable
    whose node time, `offset` later, lies inside the previous plan's horizon (offset + node_time <= T + 1e-9) is the
    previous plan's spline of its set at min(offset + node_time, T), derivative is_vel, component dim; every other free
    variable is straight_line[v].  offset + node_time is the float64 sum (data, as k / hz is in sample_rows)."""
    fixed_mask = np.asarray(fixed_mask, bool)
    out = np.asarray(straight_line, np.float64).astype(dtype)
    out[fixed_mask] = np.asarray(fixed_values, np.float64).astype(dtype)[fixed_mask]
    inside = shifted_mask(L, offset, fixed_mask)
    t = np.minimum(np.float64(offset) + L.node_time, L.T)
    for s in range(N_SETS):
        for q in range(2):
            v = np.nonzero(inside & (L.var_set == s) & (L.var_is_vel == q))[0]
            if len(v):
                out[v] = eval_spline(L, s, x_prev, t[v], q, dtype)[np.arange(len(v)), L.var_dim[v]]
    return out


def table_cell(dx, dy, start, goal):
    """Cell and weights of a goal displacement in the table's grid: (i0, i1, j0, j1, wx, wy), float64 -- the weights are
    the data the interpolation starts from.  The displacement is clamped to the grid; a grid of one line has weight 0."""
    dx, dy = np.asarray(dx, np.float64), np.asarray(dy, np.float64)
    gx, gy = np.float64(goal[0]) - np.float64(start[0]), np.float64(goal[1]) - np.float64(start[1])

    def one(g, x):
        i = 0
        while i + 2 < len(x) and g >= x[i + 1]:
            i += 1
        i1 = min(i + 1, len(x) - 1)
        w = min(max((g - x[i]) / (x[i1] - x[i]), 0.0), 1.0) if i1 > i else 0.0
        return i, i1, np.float64(w)
    i0, i1, wx = one(gx, dx)
    j0, j1, wy = one(gy, dy)
    return i0, i1, j0, j1, wx, wy


def table_guess(dx, dy, nodes, start, goal, L, dtype=np.longdouble):
    """The starting point of a cold solve with a table of nominal plans, before the swing rule: nodes [len(dy), len(dx),
    n_vars] interpolated bilinearly over the goal displacement goal - start (clamped to the grid); the position variables
    of sets 0 .. 5 (CoM, Euler, feet) shifted by start[src] - table(ref), ref = the same component of the interpolated
    plan's own start; fixed variables from start / goal."""
    nodes = np.asarray(nodes, np.float64).reshape(len(dy), len(dx), L.n_vars).astype(dtype)
    i0, i1, j0, j1, wx, wy = table_cell(dx, dy, start, goal)
    wx, wy, one = dtype(wx), dtype(wy), dtype(1)
    val = (one - wy) * ((one - wx) * nodes[j0, i0] + wx * nodes[j0, i1]) + wy * ((one - wx) * nodes[j1, i0] + wx * nodes[j1, i1])
    offs = [L.off_lin, L.off_ang] + list(L.off_eem)
    out = val.copy()
    st = np.asarray(start, np.float64).astype(dtype)
    for v in np.nonzero((L.var_is_vel == 0) & (L.var_set < 6))[0]:
        s, d = L.var_set[v], L.var_dim[v]
        out[v] = val[v] + (st[3 * s + d] - val[offs[s] + d])
    mask, fv = fixed_values(L, start, goal)
    out[mask] = fv.astype(dtype)[mask]
    return out
