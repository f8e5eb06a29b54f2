"""Force fit: the contact forces of every sampled row made to supply the wrench the planned MOTION needs.  The rule of k_force_fit
(qtos_force_fit*, include/qtos_planner.h) stated in numpy.

The solver holds Newton's law at its knots; between them the 1 kHz rows do not obey it (plan_check.py measures by how much).
The motion is what the robot tracks, so the forces give: per row the wrench the feet must supply is known exactly -- it is
columns 1 .. 6 of the check row -- and the correction is distributed over the feet in stance by one small damped weighted
least-squares solve ("force distribution").  Rows are independent.

The number type is a parameter, as in plan_check.py and joints.py: dtype = np.longdouble is what the kernel is held to, np.float64
the same formulas in the kernel's own precision.  The spline layout and the constants come in as plan_check.check_rows takes them.

Per row k of a window, at the plan time min(k / hz, T), with r, p_e, f_e and stance as check_rows forms them (its rule for a row on
a phase switch included):

  rho_ang, rho_lin   the check row's columns 1 .. 3 and 4 .. 6 of the plan's own forces, formed with m_s = mass mass_scale and the
                     inertia mass_scale inertia_b -- two float64 products, data as k_rollout forms them
  S, n               the feet whose motion polynomial is a stance, and their number
  d_e                (p_e - r) / arm: the lever arm in units of `arm`, so that moment rows / arm and force rows are both newtons
  rho~               (rho_ang / arm, rho_lin)
  A~_e               [skew(d_e); I3], 6 x 3: A~_e v = (d_e x v, v)
  g_e                the first of the NLP's five force rows of f_e (normal . f_e with the terrain basis at the foot)
  w_e                max(n max(g_e, 0) / sum_S max(g, 0), w_min); all 1 where the sum is not > 0
  M                  sum_S w_e A~_e A~_e^T + damping n I6, SPD because damping > 0
  y                  M^-1 rho~ by the unpivoted 6 x 6 Cholesky below
  df_e               w_e A~_e^T y = w_e (y_ang x d_e + y_lin) for e in S
  f_fit_e            f_e + df_e for e in S; a swing foot keeps the plan's force; n = 0: nothing is fitted

The order of the operations (only +, -, x, / and sqrt), the one the kernel runs as well:
  sums over the feet in the order FL FR HL HR: W += w, s_i += w d_i, q_ij += (w d_i) d_j (i <= j); lambda = damping n
  M = [[(q11 + q22) + lambda, ., .], [-q01, (q00 + q22) + lambda, .], [-q02, -q12, (q00 + q11) + lambda],
       [0, s2, -s1, W + lambda, ., .], [-s2, 0, s0, 0, W + lambda, .], [s1, -s0, 0, 0, 0, W + lambda]]   (the lower triangle)
  Cholesky, column j = 0 .. 5: L_jj = sqrt(M_jj - L_j0^2 - .. - L_j,j-1^2), the squares taken off one after the other; below it
  L_ij = (M_ij - L_i0 L_j0 - .. - L_i,j-1 L_j,j-1) / L_jj.  Forward z_i = (rho~_i - L_i0 z_0 - .. - L_i,i-1 z_i-1) / L_ii, backward
  from i = 5: y_i = (z_i - L_i+1,i y_i+1 - .. - L_5i y_5) / L_ii.

A fit row has 32 columns (COLS):

   0         t0 + k / hz, qtos_sample_csv's time stamp of CSV row k
   1 .. 12   f_fit, feet FL FR HL HR x xyz, world frame                                                        [N]
  13 .. 15   the angular dynamics rows with f_fit in place of f: rho_ang - sum_S (p_e - r) x df_e, foot after foot  [N m], signed
  16 .. 18   the linear ones: rho_lin - sum_S df_e                                                             [N], signed
  19         sqrt(sum_S |df_e|^2), |df|^2 = (x^2 + y^2) + z^2                                                   [N]
  20 .. 31   tau_ff = -J^T R^T f_fit per leg (joints.feed_forward), J at the joint angles q in columns 1 .. 12 of the same row of
             the joint table (qtos_joint_rows' rows); without a joint table these columns are not touched (zeros here)  [N m]

and a status word: bit 0 (NO_STANCE) no stance foot; bit 1 (TWO_STANCE) exactly two stance feet -- two point feet cannot supply a
moment about the line through them, what remains is the damped least-squares compromise; bit 2 (NONFINITE) one of columns 13 ..
19 or of the df_e is not finite: then f_fit is the plan's force and columns 13 .. 19 are NaN; bit 3 + e (EXCESS << e) the fitted
force of stance foot e exceeds the NLP's five force rows by more than excess_tol (check_rows' formula of column 23 + e on f_fit).

The summary has four records per window (FAMILIES): res_ang max |13 .. 15|, res_lin max |16 .. 18|, change column 19, excess the
largest positive excess over the stance feet -- with plan_check.summarise's semantics (largest violation, lowest row that attains
it, rows over tol[f], non-finite: +inf, no rows: -inf, -1, 0) and plan_check.accumulate's merge.  The excess is not a column: it is
formed again from columns 1 .. 12 with the float64 formula one rounded operation after the other, as the kernel forms it, so the
summary is a function of the table, the stance flags and the terrain slopes under the feet -- which are zero on flat ground and on
nearest-cell terrain (terrain_mode 1), where summarise(table) equals the kernel's records to the bit.
"""
import numpy as np

from . import joints
from . import plan_check as pc

NEE = 4
COLS = 32
FAMILIES = ("res_ang", "res_lin", "change", "excess")
UNITS = ("N m", "N", "N", "N")
SUMMARY = pc.SUMMARY
ACCUMULATE = 1                                   # QTOS_FIT_ACCUMULATE
NO_STANCE, TWO_STANCE, NONFINITE, EXCESS = 1, 2, 4, 8
FIT_TOL = (1e-3, 1e-2, 5.0, 1e-2)                # the default tol per family: N m, N, N, N


class FitParams:
    """What fit_rows reads besides the planner's constants: the rule's four numbers and the leg data of the feed-forward columns.
    capi.QtosForceFit has the same field names and is taken as well.

    The defaults arm = 0.2 m, damping = 1e-6, w_min = 0.01, excess_tol = 1e-2 N come from a float64 numpy trial of this rule on three
    solved plans (a walk, a trot, a walk onto ledges; tests/test_force_fit_cpu.py measures the same figures again) and from
    nothing measured on a robot."""

    def __init__(self, arm=0.2, damping=1e-6, w_min=0.01, excess_tol=1e-2, robot=None, ee_shift=0.015):
        robot = joints.SOLO12 if robot is None else robot
        self.arm, self.damping, self.w_min, self.excess_tol = float(arm), float(damping), float(w_min), float(excess_tol)
        if not self.arm > 0 or not self.damping > 0 or not (0 < self.w_min <= 1):
            raise ValueError("arm > 0, damping > 0 and 0 < w_min <= 1")
        self.hip, self.lateral = np.array(robot.hip, np.float64).reshape(NEE, 3), np.array(robot.lateral, np.float64).reshape(NEE)
        self.l_upper, self.l_lower = float(robot.l_upper), float(robot.l_lower)
        self.knee_sign = np.array(robot.knee_sign, np.float64).reshape(NEE)
        self.ee_shift = float(ee_shift)


def fit_params(cfg=None, **kw):
    """The FitParams of a planner configuration: the defaults above (cfg carries none of them today; it is taken so that a
    configuration can bring its own later), overridden by the keywords arm, damping, w_min, excess_tol, robot, ee_shift."""
    del cfg
    return FitParams(**kw)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def system(d, w, stance, lam, dtype):
    """M [n, 6, 6] (symmetric, both triangles filled) from d [n, 4, 3], w [n, 4], stance [n, 4] and lambda [n], in the stated order."""
    n = len(d)
    zero = np.zeros(n, dtype)
    W, s, q = zero.copy(), [zero.copy() for _ in range(3)], {}
    for i in range(3):
        for j in range(i, 3):
            q[i, j] = zero.copy()
    for e in range(NEE):
        on = stance[:, e]
        we = np.where(on, w[:, e], dtype(0))
        de = np.where(on[:, None], d[:, e], dtype(0))
        W = W + we
        for i in range(3):
            wd = we * de[:, i]
            s[i] = s[i] + wd
            for j in range(i, 3):
                q[i, j] = q[i, j] + wd * de[:, j]
    M = np.zeros((n, 6, 6), dtype)
    M[:, 0, 0], M[:, 1, 1], M[:, 2, 2] = (q[1, 1] + q[2, 2]) + lam, (q[0, 0] + q[2, 2]) + lam, (q[0, 0] + q[1, 1]) + lam
    M[:, 1, 0], M[:, 2, 0], M[:, 2, 1] = -q[0, 1], -q[0, 2], -q[1, 2]
    M[:, 3, 1], M[:, 3, 2], M[:, 4, 0], M[:, 4, 2], M[:, 5, 0], M[:, 5, 1] = s[2], -s[1], -s[2], s[0], s[1], -s[0]
    M[:, 3, 3] = M[:, 4, 4] = M[:, 5, 5] = W + lam
    for i in range(6):
        for j in range(i):
            M[:, j, i] = M[:, i, j]
    return M


def cholesky_solve(M, rhs, dtype):
    """y = M^-1 rhs, M [n, 6, 6] (its lower triangle is read), rhs [n, 6]: the unpivoted Cholesky of the module's docstring."""
    n = len(M)
    L = np.zeros((n, 6, 6), dtype)
    for j in range(6):
        acc = M[:, j, j].copy()
        for k in range(j):
            acc = acc - L[:, j, k] * L[:, j, k]
        L[:, j, j] = np.sqrt(acc)
        for i in range(j + 1, 6):
            acc = M[:, i, j].copy()
            for k in range(j):
                acc = acc - L[:, i, k] * L[:, j, k]
            L[:, i, j] = acc / L[:, j, j]
    z = np.zeros((n, 6), dtype)
    for i in range(6):
        acc = rhs[:, i].copy()
        for k in range(i):
            acc = acc - L[:, i, k] * z[:, k]
        z[:, i] = acc / L[:, i, i]
    y = np.zeros((n, 6), dtype)
    for i in range(5, -1, -1):
        acc = z[:, i].copy()
        for k in range(i + 1, 6):
            acc = acc - L[:, k, i] * y[:, k]
        y[:, i] = acc / L[:, i, i]
    return y


def force_excess(f, hx, hy, mu, f_max, dtype):
    """check_rows' excess of a stance foot (its column 23 + e) of the forces f [n, 3]: the largest excess of the NLP's five force
    rows; NaN where a row is not finite."""
    fg = pc.force_rows(f, hx, hy, mu, dtype)
    f_max = dtype(np.float64(f_max))
    with np.errstate(invalid="ignore"):
        ex = np.maximum(np.maximum(np.maximum(-fg[:, 0], fg[:, 0] - f_max), np.maximum(fg[:, 1], -fg[:, 2])), np.maximum(fg[:, 3], -fg[:, 4]))
    return np.where(np.isfinite(fg).all(axis=1), ex, dtype(np.nan))


def fit_rows(L, nodes, t0, hz, first_row, n_rows, params, fit=None, terrain=None, mass_scale=1.0, joint=None, times=None,
             dtype=np.float64, detail=False):
    """The fit rows first_row .. first_row + n_rows - 1 of the plan `nodes` [n_vars]: ([n_rows, 32] in dtype, status [n_rows] int32;
    the module's docstring has the columns and the bits).  params: the planner's constants as check_rows takes them; fit: a
    FitParams (None: the defaults); terrain: (height_xy, cell, x0, y0) of the window's map, None for flat ground; mass_scale: the
    window's, as k_rollout scales mass and inertia; joint: [n_rows, 37] float64 joint rows of the same rows (None: columns 20 .. 31
    stay zero); times: the rows are at exactly these plan times instead.  detail: also a dict -- rho [n, 6] the plan's own dynamics
    rows, d [n, 4, 3], w [n, 4], stance [n, 4], M [n, 6, 6], y [n, 6], df [n, 4, 3], excess [n, 4] (NaN for a swing foot), slopes
    [n, 4, 2], p [n, 4, 3], r, a, th, thd, thdd [n, 3] and f [n, 4, 3] the plan's forces."""
    fit = FitParams() if fit is None else fit
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return _fit_rows(L, nodes, t0, hz, first_row, n_rows, params, fit, terrain, mass_scale, joint, times, dtype, detail)


def _fit_rows(L, nodes, t0, hz, first_row, n_rows, params, fit, terrain, mass_scale, joint, times, dtype, detail):
    off, t = pc.row_times(L, hz, first_row, n_rows, times)
    n = len(t)
    sp = L.splines
    x = np.asarray(nodes, np.float64).reshape(-1)
    out = np.zeros((n, COLS), dtype)
    out[:, 0] = dtype(np.float64(t0)) + off.astype(dtype)
    r, a = pc.eval_spline(sp[0], x, t, 0, dtype), pc.eval_spline(sp[0], x, t, 2, dtype)
    th, thd, thdd = pc.eval_spline(sp[1], x, t, 0, dtype), pc.eval_spline(sp[1], x, t, 1, dtype), pc.eval_spline(sp[1], x, t, 2, dtype)
    ms = np.float64(mass_scale)
    mass, grav = dtype(np.float64(params.mass) * ms), dtype(np.float64(params.gravity))            # (float64 products: data)
    Ib = ms * np.asarray(params.inertia_b, np.float64).reshape(3, 3)
    rho_ang = pc.dyn_angular(Ib, th, thd, thdd, dtype)
    rho_lin = mass * a
    rho_lin[:, 2] = rho_lin[:, 2] + mass * grav
    stance = pc.stance_rows(L, hz, first_row, n_rows, times)
    mode = int(getattr(params, "terrain_mode", 0))
    arm, w_min = dtype(np.float64(fit.arm)), dtype(np.float64(fit.w_min))
    p, f, g = np.empty((n, NEE, 3), dtype), np.empty((n, NEE, 3), dtype), np.empty((n, NEE), dtype)
    slopes = np.empty((n, NEE, 2), dtype)
    for e in range(NEE):
        pe, fe = pc.eval_spline(sp[2 + e], x, t, 0, dtype), pc.eval_spline(sp[6 + e], x, t, 0, dtype)
        rho_ang = rho_ang - _cross(fe, r - pe)
        rho_lin = rho_lin - fe
        _, hx, hy = pc.terrain_at(terrain, mode, pe[:, 0], pe[:, 1], dtype)
        p[:, e], f[:, e], slopes[:, e, 0], slopes[:, e, 1] = pe - r, fe, hx, hy
        g[:, e] = pc.force_rows(fe, hx, hy, params.friction, dtype)[:, 0]
    # weights
    cnt = stance.sum(axis=1)
    nn = cnt.astype(dtype)
    gpos = np.where(stance & (g > 0), g, dtype(0))
    gsum = ((gpos[:, 0] + gpos[:, 1]) + gpos[:, 2]) + gpos[:, 3]
    loaded = gsum > 0
    w = np.where(loaded[:, None], np.maximum((nn[:, None] * gpos) / np.where(loaded, gsum, dtype(1))[:, None], w_min), dtype(1))
    # the system and its solve (rows without a stance foot: nothing is fitted)
    d = p / arm
    lam = dtype(np.float64(fit.damping)) * nn
    rho_s = np.concatenate([rho_ang / arm, rho_lin], axis=1)
    M = system(d, w, stance, lam, dtype)
    some = cnt > 0
    Ms = np.where(some[:, None, None], M, np.eye(6, dtype=dtype)[None])
    y = np.where(some[:, None], cholesky_solve(Ms, rho_s, dtype), dtype(0))
    df = np.zeros((n, NEE, 3), dtype)
    res_ang, res_lin, sq = rho_ang.copy(), rho_lin.copy(), np.zeros(n, dtype)
    for e in range(NEE):
        on = stance[:, e]
        de = (_cross(y[:, 0:3], d[:, e]) + y[:, 3:6]) * w[:, e][:, None]
        de = np.where(on[:, None], de, dtype(0))
        df[:, e] = de
        res_ang = res_ang - _cross(p[:, e], de)
        res_lin = res_lin - de
        sq = sq + ((de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]) + de[:, 2] * de[:, 2])
    change = np.sqrt(sq)
    bad = ~(np.isfinite(res_ang).all(axis=1) & np.isfinite(res_lin).all(axis=1) & np.isfinite(change) & np.isfinite(df).all(axis=(1, 2)))
    f_fit = np.where(bad[:, None, None], f, f + df)
    f_fit = np.where(stance[:, :, None], f_fit, f)                                                  # (a swing foot: the plan's force, to the bit)
    nan = np.where(bad, dtype(np.nan), dtype(0))
    out[:, 1:13] = f_fit.reshape(n, 12)
    out[:, 13:16], out[:, 16:19], out[:, 19] = res_ang + nan[:, None], res_lin + nan[:, None], change + nan
    status = np.where(cnt == 0, NO_STANCE, 0) | np.where(cnt == 2, TWO_STANCE, 0) | np.where(bad, NONFINITE, 0)
    excess = np.full((n, NEE), np.nan, dtype)
    tol = dtype(np.float64(fit.excess_tol))
    for e in range(NEE):
        ex = force_excess(f_fit[:, e], slopes[:, e, 0], slopes[:, e, 1], params.friction, params.force_limit, dtype)
        excess[:, e] = np.where(stance[:, e], ex, dtype(np.nan))
        status = status | np.where(stance[:, e] & (ex > tol), EXCESS << e, 0)
    if joint is not None:
        q = np.asarray(joint, np.float64).reshape(n, joints.JOINT_COLS)[:, 1:13]
        for e in range(NEE):
            out[:, 20 + 3 * e:23 + 3 * e] = joints.feed_forward(e, q[:, 3 * e:3 * e + 3], th, f_fit[:, e], fit, dtype)
    status = status.astype(np.int32)
    if detail:
        return out, status, dict(rho=np.concatenate([rho_ang, rho_lin], axis=1), d=d, w=w, stance=stance, M=M, y=y, df=df, excess=excess,
                                 slopes=slopes, p=p, r=r, a=a, th=th, thd=thd, thdd=thdd, f=f)
    return out, status


def violations(table, stance, params, slopes=None):
    """[n, 4] float64: the violation of every family per row of a float64 table; a non-finite column counts as +inf.  The excess
    is formed from columns 1 .. 12 in float64 (slopes [n, 4, 2]: the terrain's hx, hy under the feet; None: zero)."""
    T = np.asarray(table, np.float64).reshape(-1, COLS)
    n = len(T)
    stance = np.asarray(stance, bool).reshape(n, NEE)
    inf = np.float64(np.inf)
    fin = np.isfinite(T)
    v = np.zeros((n, 4))
    v[:, 0] = np.where(fin[:, 13:16], np.abs(T[:, 13:16]), inf).max(axis=1, initial=0.0)
    v[:, 1] = np.where(fin[:, 16:19], np.abs(T[:, 16:19]), inf).max(axis=1, initial=0.0)
    v[:, 2] = np.where(fin[:, 19], np.abs(T[:, 19]), inf)
    sl = np.zeros((n, NEE, 2)) if slopes is None else np.asarray(slopes, np.float64).reshape(n, NEE, 2)
    for e in range(NEE):
        ex = force_excess(T[:, 1 + 3 * e:4 + 3 * e], sl[:, e, 0], sl[:, e, 1], params.friction, params.force_limit, np.float64)
        ve = np.where(np.isfinite(ex), np.where(ex > 0, ex, 0.0), inf)
        v[:, 3] = np.maximum(v[:, 3], np.where(stance[:, e], ve, 0.0))
    return v


def empty_summary(*shape):
    """[*shape, 4] records that nothing has been merged into: max -inf, row -1, count 0."""
    s = np.zeros(tuple(shape) + (4,), SUMMARY)
    s["max"], s["row"] = -np.inf, -1
    return s


def summarise(table, first_row, stance, tol, params, slopes=None):
    """The four families of a float64 table [n, 32] as four SUMMARY records, with plan_check.summarise's semantics: max the largest
    violation, row the lowest row that attains it, counted from first_row (-1 where n = 0, with max -inf), count the rows with a
    violation > tol[f]."""
    v = violations(table, stance, params, slopes)
    out = empty_summary()
    tol = np.asarray(tol, np.float64).reshape(4)
    if len(v):
        out["max"] = v.max(axis=0)
        out["row"] = np.int64(first_row) + np.argmax(v == out["max"][None, :], axis=0)
        out["count"] = (v > tol[None, :]).sum(axis=0)
    return out


accumulate = pc.accumulate           # QTOS_FIT_ACCUMULATE merges as QTOS_CHECK_ACCUMULATE does


def report_lines(summary, t0=0.0, hz=1000.0, tol=None):
    """One line per family of four SUMMARY records, in plan_check.report_lines' format."""
    lines = []
    for i, name in enumerate(FAMILIES):
        s = summary[i]
        when = "-" if s["row"] < 0 else "%.3f s (row %d)" % (float(t0) + int(s["row"]) / float(hz), int(s["row"]))
        over = "" if tol is None else " over %.1e" % float(tol[i])
        lines.append("force fit  %-8s max %.3e %-3s at %s, %d rows%s" % (name, float(s["max"]), UNITS[i], when, int(s["count"]), over))
    return lines
