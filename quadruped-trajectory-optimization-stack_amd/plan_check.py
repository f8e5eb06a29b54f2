"""Plan check: what a plan violates between its knots.  The rule of k_plan_check (qtos_plan_check*, include/qtos_planner.h)
stated in numpy.

The solver enforces the rows of its NLP at their own times only: the dynamics every dt_dynamic, the range of motion every
dt_range_of_motion, the terrain at the foot nodes, friction and the unilateral force at the force nodes.  What the robot
executes are the 1 kHz rows in between.  check_rows evaluates the same rows at every sampled time, summarise reduces the
table to five families, accumulate merges the summaries of the segments a receding loop executed.

The number type is a parameter, as in joints.py: dtype = np.longdouble is what the kernel is held to, np.float64 the same
formulas in the kernel's own precision.  The package does not import the oracle: the spline layout comes in as an
argument (an object with .splines -- ten records with .dur, .idx [n_polys + 1, 2, 3] and .n_polys: lin, ang, the four foot
motions, the four foot forces -- and .T), and the constants as a PlannerConfig (or anything with its field names: mass,
gravity, inertia_b, nominal_stance, max_deviation, friction, force_limit, terrain_mode).

A check row has 27 columns:

   0        t0 + k / hz, qtos_sample_csv's time stamp of CSV row k
   1 ..  3  angular dynamics rows  I_w wd + w x (I_w w) - sum_e f_e x (r - p_e)                     [N m], signed
   4 ..  6  linear dynamics rows   m a + m g e_z - sum_e f_e                                        [N], signed
   7 .. 18  range of motion, feet FL FR HL HR x 3 axes: max(lo - g, g - hi) of g = R^T (p_e - r) against lo, hi =
            nominal_stance -+ max_deviation; negative: inside                                      [m]
  19 .. 22  clearance of the feet z - h(x, y) under the terrain mode and the window's map (flat ground without one)    [m]
  23 .. 26  force excess of the feet.  Stance polynomial: the largest excess of the five force rows of the NLP -- the
            normal force in [0, f_max], t1 - mu n <= 0, t1 + mu n >= 0, t2 - mu n <= 0, t2 + mu n >= 0 -- with the
            terrain basis at the foot's position.  Swing polynomial: max |f_i|                       [N]

The plan time of row k is min(k / hz, T).  A time within 1e-10 s behind a junction of a spline belongs to the polynomial
in front of it (sample_spline's rule); stance or swing is a property of the foot-motion polynomial.
"""
import numpy as np

NEE = 4
COLS = 27
FAMILIES = ("dyn_ang", "dyn_lin", "rom", "terrain", "force")
SUMMARY = np.dtype([("max", np.float64), ("row", np.int64), ("count", np.int64)])    # one record of d_summary
ACCUMULATE = 1                                                                       # QTOS_CHECK_ACCUMULATE
LOCATE_EPS = 1e-10


def _poly_of(S, t):
    """The polynomial of the float64 times t: the first whose float64 end is >= t - 1e-10 (the times are data: one choice for
    every number type)."""
    tend = np.cumsum(np.asarray(S.dur, np.float64))
    return np.minimum(np.searchsorted(tend, np.asarray(t, np.float64) - LOCATE_EPS, side="left"), S.n_polys - 1)


def _hermite_w(T, t, deriv):
    T2 = T * T
    T3 = T2 * T
    t2 = t * t
    t3 = t2 * t
    if deriv == 0:
        return (1 - 3 * t2 / T2 + 2 * t3 / T3, t - 2 * t2 / T + t3 / T2, 3 * t2 / T2 - 2 * t3 / T3, -t2 / T + t3 / T2)
    if deriv == 1:
        return (-6 * t / T2 + 6 * t2 / T3, 1 - 4 * t / T + 3 * t2 / T2, 6 * t / T2 - 6 * t2 / T3, -2 * t / T + 3 * t2 / T2)
    return (-6 / T2 + 12 * t / T3, -4 / T + 6 * t / T2, 6 / T2 - 12 * t / T3, -2 / T + 6 * t / T2)


def eval_spline(S, x, t, deriv, dtype=np.float64):
    """Spline S of the node vector x at the float64 times t, value or first or second derivative: [n, 3] in dtype.  The local
    time is t - (end - duration) of the polynomial, the end the running sum of the durations (sample_spline's form)."""
    t = np.atleast_1d(np.asarray(t, np.float64))
    k = _poly_of(S, t)
    dur = np.asarray(S.dur, np.float64).astype(dtype)
    ends = np.cumsum(dur, dtype=dtype)
    tau = t.astype(dtype) - (ends[k] - dur[k])
    w = _hermite_w(dur[k], tau, deriv)
    idx = np.asarray(S.idx, np.int64).reshape(S.n_polys + 1, 2, 3)
    x = np.asarray(x, np.float64).astype(dtype)
    out = np.zeros((len(t), 3), dtype)
    for d in range(3):
        acc = np.zeros(len(t), dtype)
        for a in range(4):
            var = idx[k + (a >> 1), a & 1, d]
            acc = acc + w[a] * np.where(var >= 0, x[np.maximum(var, 0)], dtype(0))
        out[:, d] = acc
    return out


def stance_table(S):
    """Per polynomial of a foot-motion spline: True for a stance (neither of its nodes has a velocity variable)."""
    idx = np.asarray(S.idx, np.int64).reshape(S.n_polys + 1, 2, 3)
    return (idx[:-1, 1, 0] < 0) & (idx[1:, 1, 0] < 0)


def row_times(L, hz, first_row, n_rows, times=None):
    """(stamp offsets, plan times) of the rows, float64: k / hz and min(k / hz, T); with `times` those, unclamped."""
    if times is not None:
        t = np.asarray(times, np.float64).reshape(-1)
        return t, t
    k = np.float64(first_row) + np.arange(int(n_rows), dtype=np.float64)
    tk = k / np.float64(hz)
    return tk, np.minimum(tk, np.float64(L.T))


def stance_rows(L, hz, first_row, n_rows, times=None):
    """[n, 4] bool: whether foot e's motion polynomial at the row's plan time is a stance."""
    _, t = row_times(L, hz, first_row, n_rows, times)
    return np.stack([stance_table(L.splines[2 + e])[_poly_of(L.splines[2 + e], t)] for e in range(NEE)], axis=1)


def rotation(th, dtype):
    """R = Rz(yaw) Ry(pitch) Rx(roll), th = (roll, pitch, yaw) [n, 3]: [n, 3, 3]."""
    sx, cx, sy, cy, sz, cz = np.sin(th[:, 0]), np.cos(th[:, 0]), np.sin(th[:, 1]), np.cos(th[:, 1]), np.sin(th[:, 2]), np.cos(th[:, 2])
    R = np.empty((len(th), 3, 3), dtype)
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = cy * cz, cz * sx * sy - cx * sz, sx * sz + cx * cz * sy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = cy * sz, cx * cz + sx * sy * sz, cx * sy * sz - cz * sx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = -sy, cy * sx, cx * cy
    return R


def dyn_angular(Ib, th, thd, thdd, dtype):
    """I_w wd + w x (I_w w) with I_w = R Ib R^T, w = M(th) thd, wd = Mdot thd + M thdd: [n, 3]."""
    sy, cy, sz, cz = np.sin(th[:, 1]), np.cos(th[:, 1]), np.sin(th[:, 2]), np.cos(th[:, 2])
    yd, zd = thd[:, 1], thd[:, 2]
    w = np.stack([cy * cz * thd[:, 0] - sz * thd[:, 1], cy * sz * thd[:, 0] + cz * thd[:, 1], thd[:, 2] - sy * thd[:, 0]], axis=1)
    m00, m01 = -(cz * sy * yd) - cy * sz * zd, -(cz * zd)
    m10, m11 = cy * cz * zd - sy * sz * yd, -(sz * zd)
    m20 = -(cy * yd)
    wd = np.stack([m00 * thd[:, 0] + m01 * thd[:, 1] + cy * cz * thdd[:, 0] - sz * thdd[:, 1],
                   m10 * thd[:, 0] + m11 * thd[:, 1] + cy * sz * thdd[:, 0] + cz * thdd[:, 1],
                   m20 * thd[:, 0] + thdd[:, 2] - sy * thdd[:, 0]], axis=1)
    R = rotation(th, dtype)
    Ib = np.asarray(Ib, np.float64).reshape(3, 3).astype(dtype)
    u, ud = np.einsum("nji,nj->ni", R, w), np.einsum("nji,nj->ni", R, wd)          # R^T w, R^T wd
    Iww, Iwd = np.einsum("nij,nj->ni", R, u @ Ib.T), np.einsum("nij,nj->ni", R, ud @ Ib.T)
    return Iwd + np.cross(w, Iww)


def terrain_at(terrain, mode, x, y, dtype):
    """(h, hx, hy) of the heightfield under x, y [n]: terrain = (height_xy [nx, ny], cell, x0, y0) or None for flat ground;
    mode 1 the nearest cell, mode 0 bilinear with zero slope where the point is clamped to the border.  A point at a non-finite
    place has no terrain: NaN, on flat ground as well."""
    zero = np.zeros(len(x), dtype)
    if terrain is None:
        nan = np.where(np.isfinite(x) & np.isfinite(y), dtype(0), dtype(np.nan))
        return nan, nan, nan
    H, cell, x0, y0 = terrain
    H = np.asarray(H, np.float64)
    nx, ny = H.shape
    Hd = H.astype(dtype)
    fx, fy = (x - dtype(np.float64(x0))) / dtype(np.float64(cell)), (y - dtype(np.float64(y0))) / dtype(np.float64(cell))
    bad = ~(np.isfinite(fx) & np.isfinite(fy))
    fx, fy = np.where(bad, dtype(0), fx), np.where(bad, dtype(0), fy)
    nan = np.where(bad, dtype(np.nan), dtype(0))
    if mode == 1:
        # clipped in floating point, then converted: beyond 2^63 the conversion is not defined (numpy gives the FIRST cell)
        jx = np.clip(np.floor(fx + dtype(0.5)), 0, nx - 1).astype(np.int64)
        jy = np.clip(np.floor(fy + dtype(0.5)), 0, ny - 1).astype(np.int64)
        return Hd[jx, jy] + nan, zero + nan, zero + nan
    cx, cy = (fx <= 0) | (fx >= nx - 1), (fy <= 0) | (fy >= ny - 1)
    fx, fy = np.clip(fx, 0, nx - 1), np.clip(fy, 0, ny - 1)
    ix = np.clip(np.floor(fx).astype(np.int64), 0, max(nx - 2, 0))
    iy = np.clip(np.floor(fy).astype(np.int64), 0, max(ny - 2, 0))
    u, v = fx - ix, fy - iy
    ix1, iy1 = (ix + 1 if nx > 1 else ix), (iy + 1 if ny > 1 else iy)
    h00, h10, h01, h11 = Hd[ix, iy], Hd[ix1, iy], Hd[ix, iy1], Hd[ix1, iy1]
    h = h00 * (1 - u) * (1 - v) + h10 * u * (1 - v) + h01 * (1 - u) * v + h11 * u * v
    c = dtype(np.float64(cell))
    hx = np.where(cx, dtype(0), ((h10 - h00) * (1 - v) + (h11 - h01) * v) / c)
    hy = np.where(cy, dtype(0), ((h01 - h00) * (1 - u) + (h11 - h10) * u) / c)
    return h + nan, hx + nan, hy + nan


def force_rows(f, hx, hy, mu, dtype):
    """The five force rows of the NLP [n, 5] of the forces f [n, 3] on a terrain with the slopes hx, hy [n]: n . f, then
    (t1 - mu n) . f, (t1 + mu n) . f, (t2 - mu n) . f, (t2 + mu n) . f with the normalised normal and tangents."""
    one, zero = np.ones(len(f), dtype), np.zeros(len(f), dtype)
    basis = []
    for v in ((-hx, -hy, one), (one, zero, hx), (zero, one, hy)):
        nn = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        basis.append(np.stack([v[0] / nn, v[1] / nn, v[2] / nn], axis=1))
    mu = dtype(np.float64(mu))
    out = np.empty((len(f), 5), dtype)
    for row, (cn, c1, c2) in enumerate(((1, 0, 0), (-mu, 1, 0), (mu, 1, 0), (-mu, 0, 1), (mu, 0, 1))):
        v = cn * basis[0] + c1 * basis[1] + c2 * basis[2]
        out[:, row] = f[:, 0] * v[:, 0] + f[:, 1] * v[:, 1] + f[:, 2] * v[:, 2]
    return out


def rom_bounds(params):
    """(lo, hi) [4, 3] of the range-of-motion rows, float64: nominal_stance -+ max_deviation."""
    nom = np.asarray(params.nominal_stance, np.float64).reshape(NEE, 3)
    dev = np.asarray(params.max_deviation, np.float64).reshape(3)
    return nom - dev, nom + dev


def check_rows(L, nodes, t0, hz, first_row, n_rows, params, terrain=None, times=None, dtype=np.float64, detail=False):
    """The check rows first_row .. first_row + n_rows - 1 of the plan `nodes` [n_vars]: [n_rows, 27] in dtype (the module's
    docstring has the columns).  times: the rows are at exactly these plan times instead (column 0: t0 + time).  terrain:
    (height_xy [nx, ny], cell, x0, y0) of the window's map, None for flat ground.  detail: also a dict with what stands behind
    the excess columns -- rom_g [n, 12] the range-of-motion row values, force_g [n, 4, 5] the five force rows of every foot
    (whatever its phase), stance [n, 4]."""
    off, t = row_times(L, hz, first_row, n_rows, times)
    n = len(t)
    sp = L.splines
    x = np.asarray(nodes, np.float64).reshape(-1)
    out = np.empty((n, COLS), dtype)
    out[:, 0] = dtype(np.float64(t0)) + off.astype(dtype)
    r, a = eval_spline(sp[0], x, t, 0, dtype), eval_spline(sp[0], x, t, 2, dtype)
    th, thd, thdd = eval_spline(sp[1], x, t, 0, dtype), eval_spline(sp[1], x, t, 1, dtype), eval_spline(sp[1], x, t, 2, dtype)
    mass, grav = dtype(np.float64(params.mass)), dtype(np.float64(params.gravity))
    g_ang = dyn_angular(params.inertia_b, th, thd, thdd, dtype)
    g_lin = mass * a
    g_lin[:, 2] = g_lin[:, 2] + mass * grav
    R = rotation(th, dtype)
    lo, hi = rom_bounds(params)
    stance = stance_rows(L, hz, first_row, n_rows, times)
    mode = int(getattr(params, "terrain_mode", 0))
    f_max = dtype(np.float64(params.force_limit))
    rom_g, force_g = np.empty((n, 3 * NEE), dtype), np.empty((n, NEE, 5), dtype)
    for e in range(NEE):
        pe, f = eval_spline(sp[2 + e], x, t, 0, dtype), eval_spline(sp[6 + e], x, t, 0, dtype)
        d = r - pe
        g_ang = g_ang - np.cross(f, d)
        g_lin = g_lin - f
        g = np.einsum("nji,nj->ni", R, pe - r)
        rom_g[:, 3 * e:3 * e + 3] = g
        out[:, 7 + 3 * e:10 + 3 * e] = np.maximum(lo[e].astype(dtype) - g, g - hi[e].astype(dtype))
        h, hx, hy = terrain_at(terrain, mode, pe[:, 0], pe[:, 1], dtype)
        out[:, 19 + e] = pe[:, 2] - h
        fg = force_rows(f, hx, hy, params.friction, dtype)
        force_g[:, e] = fg
        ex = np.maximum(np.maximum(np.maximum(-fg[:, 0], fg[:, 0] - f_max), np.maximum(fg[:, 1], -fg[:, 2])),
                        np.maximum(fg[:, 3], -fg[:, 4]))
        sw = np.maximum(np.maximum(np.abs(f[:, 0]), np.abs(f[:, 1])), np.abs(f[:, 2]))
        nonfinite = ~np.isfinite(fg).all(axis=1)                  # (np.maximum passes a NaN on, the kernel's fmax does not)
        out[:, 23 + e] = np.where(stance[:, e], np.where(nonfinite, dtype(np.nan), ex), sw)
    out[:, 1:4], out[:, 4:7] = g_ang, g_lin
    if detail:
        return out, dict(rom_g=rom_g, force_g=force_g, stance=stance, rom_lo=lo, rom_hi=hi)
    return out


def violations(table, stance):
    """[n, 5] float64: the violation of every family per row of a float64 table; a non-finite column counts as +inf.
    stance [n, 4]: the terrain family is |clearance| of a foot in stance and max(-clearance, 0) of one in swing."""
    T = np.asarray(table, np.float64).reshape(-1, COLS)
    stance = np.asarray(stance, bool).reshape(len(T), NEE)
    inf = np.float64(np.inf)
    fin = np.isfinite(T)
    v = np.empty((len(T), 5))
    v[:, 0] = np.where(fin[:, 1:4], np.abs(T[:, 1:4]), inf).max(axis=1, initial=0.0)
    v[:, 1] = np.where(fin[:, 4:7], np.abs(T[:, 4:7]), inf).max(axis=1, initial=0.0)
    v[:, 2] = np.where(fin[:, 7:19], np.maximum(T[:, 7:19], 0.0), inf).max(axis=1, initial=0.0)
    c = T[:, 19:23]
    v[:, 3] = np.where(fin[:, 19:23], np.where(stance, np.abs(c), np.maximum(-c, 0.0)), inf).max(axis=1, initial=0.0)
    v[:, 4] = np.where(fin[:, 23:27], np.maximum(T[:, 23:27], 0.0), inf).max(axis=1, initial=0.0)
    return v


def empty_summary(*shape):
    """[*shape, 5] records that nothing has been merged into: max -inf, row -1, count 0 (what an accumulating check starts
    from, and what a check of no rows writes)."""
    s = np.zeros(tuple(shape) + (5,), SUMMARY)
    s["max"], s["row"] = -np.inf, -1
    return s


def summarise(table, first_row, stance, tol):
    """The five families of a float64 table [n, 27] as five SUMMARY records: max the largest violation, row the lowest row
    that attains it, counted from first_row (-1 where n = 0, with max -inf), count the rows with a violation > tol[f]."""
    v = violations(table, stance)
    out = empty_summary()
    tol = np.asarray(tol, np.float64).reshape(5)
    if len(v):
        out["max"] = v.max(axis=0)
        out["row"] = np.int64(first_row) + np.argmax(v == out["max"][None, :], axis=0)
        out["count"] = (v > tol[None, :]).sum(axis=0)
    return out


def accumulate(old, new):
    """QTOS_CHECK_ACCUMULATE: max = max(old, new), row replaced only on a strictly greater max, count += new."""
    old, new = np.asarray(old, SUMMARY), np.asarray(new, SUMMARY)
    out = old.copy()
    take = new["max"] > old["max"]
    out["max"] = np.where(take, new["max"], old["max"])
    out["row"] = np.where(take, new["row"], old["row"])
    out["count"] = old["count"] + new["count"]
    return out


def report_lines(summary, t0=0.0, hz=1000.0, tol=None, units=("N m", "N", "m", "m", "N")):
    """One line per family of five SUMMARY records: the max, the time of the row that attains it, the rows over tol."""
    lines = []
    for i, name in enumerate(FAMILIES):
        s = summary[i]
        when = "-" if s["row"] < 0 else "%.3f s (row %d)" % (float(t0) + int(s["row"]) / float(hz), int(s["row"]))
        over = "" if tol is None else " over %.1e" % float(tol[i])
        lines.append("plan check %-8s max %.3e %-3s at %s, %d rows%s" % (name, float(s["max"]), units[i], when, int(s["count"]), over))
    return lines
