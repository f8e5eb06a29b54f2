"""Rollout: the windows' robots as simulated rigid bodies.  The rule of k_rollout (qtos_rollout*, include/qtos_planner.h) stated
in numpy.

In the reference the robot is PyBullet: scripts/run.py steps the simulator once per 1 kHz tick and reads ``traj_vec`` back.  The
model the planner itself uses is a single rigid body -- mass, inertia_b, gravity, forces at the feet -- and this module integrates
that body forward under a plan's forces, with a PD wrench towards the plan and an optional push.  What comes out is the
measured ring k_track and k_start_feedback read.  It is NOT a simulator of the robot: no contacts, no legs' inertia, no
friction limits on the applied forces; the feet push where the plan says they stand, whether or not the body is there.

The number type is a parameter, as in plan_check.py, tracking.py and joints.py: dtype = np.longdouble is what the kernel is held
to, np.float64 the same formulas in the kernel's own order, one rounded operation after the other.  The package does not import
the oracle: the spline layout comes in as an argument (plan_check.py's docstring).

Per row k of a window the plan time is min(k / hz, T); with c the 37-column CSV row there (qtos_sample_csv's), plan_inputs forms

    r_p = c[1:4], v_p = c[19:22]
    q_p   the quaternion (x, y, z, w) of Rz Ry Rx of c[4:7], by the half-angle products
    w_p   M(th) thd, plan_check.dyn_angular's w: world frame
    F     ff_scale (((f_0 + f_1) + f_2) + f_3)
    tau_p ff_scale (((d_0 x f_0 + d_1 x f_1) + d_2 x f_2) + d_3 x f_3), d_e = p_e - r_p: about the PLANNED CoM (about the world
          origin the torques would cancel digits at x = 50 m)

The state of a window is 13 numbers: r[3], v[3] in the world, q[4] body to world (x, y, z, w), w_b[3] the angular velocity in
the body frame.  One tick takes `substeps` steps of h = 1 / (hz substeps) with the row's quantities held (zero-order hold);
`step` is one of them, every line evaluated from the state at the step's start:

     1  e = r - r_p
     2  F_fb = clip(-(kp_lin e) - kd_lin (v - v_p), +-f_fb_max) per component (a limit of 0: no clip)
     3  a = ((F + F_fb) + F_push) / m_s - g e_z,  m_s = mass mass_scale
     4  R = R(q), from products of the quaternion's components
     5  q_e = q_p (x) conj(q), negated if its w < 0
     6  e_R = 2 vec(q_e)
     7  tau_fb = clip(kp_ang e_R + kd_ang (w_p - R w_b), +-t_fb_max)
     8  tau = ((tau_p - e x F) + tau_fb) + tau_push
     9  v += h a, then r += h v (semi-implicit)
    10  w_b += h Ib_s^-1 (R^T tau - w_b x (Ib_s w_b)),  Ib_s = mass_scale inertia_b, Ib_s^-1 = inertia_b_inv / mass_scale
    11  q = (q + (h / 2) q (x) (w_b, 0)) / |.|, with the new w_b

Only +, -, x, / and sqrt.  Row k holds the state at the START of tick k.  Status bits of a row: FALLEN |e| > dev_max or
2 |vec(q_e)| > tilt_max (a limit of 0: never); NONFINITE a state that is not finite; both are sticky in the window's carried
word: the row that sets one and every later row carry it, make no step, and repeat the frozen state; GIMBAL the clip of the Euler
extraction acts; CLIPPED a feedback component was clipped in a step of this tick; PUSH the push acts in this tick: the ticks c
with push_from <= c < push_from + push_ticks, c = count + j the window's running tick count.  A frozen row has neither CLIPPED nor
PUSH, and 0 in column 19.  The carried word has one more bit, PENDING: a window that carries it is set on its plan (as by
QTOS_ROLLOUT_INIT) by the first call that gives it rows, which clears the bit; a call with no rows for the window keeps it.
"""
import numpy as np

from . import plan_check

NEE = 4
ROW_COLS = 20
STATE = 13
FALLEN, NONFINITE, GIMBAL, CLIPPED, PUSH = 1, 2, 4, 8, 16     # status bits of a row
FLAG_INIT, FLAG_QUAT = 1, 2                                  # QtosRollout.flags: QTOS_ROLLOUT_INIT, QTOS_ROLLOUT_QUAT
PENDING = 32                                                 # QTOS_ROLLOUT_PENDING: in a window's carried word, never in a row's status
INPUTS = 20                                                  # plan_inputs' columns: stamp, r_p, v_p, q_p, w_p, F, tau_p


def invert_inertia(inertia_b):
    """inertia_b^-1 [3, 3] in float64, by the adjugate; raises ValueError for a singular (or non-finite) matrix."""
    a = np.asarray(inertia_b, np.float64).reshape(3, 3)
    c = np.array([[a[1, 1] * a[2, 2] - a[1, 2] * a[2, 1], a[0, 2] * a[2, 1] - a[0, 1] * a[2, 2], a[0, 1] * a[1, 2] - a[0, 2] * a[1, 1]],
                  [a[1, 2] * a[2, 0] - a[1, 0] * a[2, 2], a[0, 0] * a[2, 2] - a[0, 2] * a[2, 0], a[0, 2] * a[1, 0] - a[0, 0] * a[1, 2]],
                  [a[1, 0] * a[2, 1] - a[1, 1] * a[2, 0], a[0, 1] * a[2, 0] - a[0, 0] * a[2, 1], a[0, 0] * a[1, 1] - a[0, 1] * a[1, 0]]])
    det = a[0, 0] * c[0, 0] + a[0, 1] * c[1, 0] + a[0, 2] * c[2, 0]
    scale = np.abs(a).max() ** 3
    if not np.isfinite(det) or not np.isfinite(scale) or abs(det) <= 1e-12 * scale:
        raise ValueError("inertia_b is singular")
    return c / det


class RolloutParams:
    """What the rule reads.  capi.QtosRollout has the same field names and is taken as well.  cfg: anything with mass, gravity
    and inertia_b (a PlannerConfig); the keywords of the same names replace its values."""

    def __init__(self, cfg=None, mass=None, gravity=None, inertia_b=None, substeps=1, ff_scale=1.0, kp_lin=0.0, kd_lin=0.0, kp_ang=0.0,
                 kd_ang=0.0, f_fb_max=0.0, t_fb_max=0.0, dev_max=0.0, tilt_max=0.0, push_from=0, push_ticks=0, quaternion=False):
        if cfg is None:
            from .config import PlannerConfig
            cfg = PlannerConfig()
        self.mass = float(cfg.mass if mass is None else mass)
        self.gravity = float(cfg.gravity if gravity is None else gravity)
        self.inertia_b = np.array(cfg.inertia_b if inertia_b is None else inertia_b, np.float64).reshape(9)
        self.inertia_b_inv = invert_inertia(self.inertia_b).reshape(9)
        self.substeps, self.ff_scale = int(substeps), float(ff_scale)
        if self.substeps < 1 or not self.mass > 0:
            raise ValueError("substeps >= 1 and mass > 0")
        three = lambda v: np.broadcast_to(np.asarray(v, np.float64), (3,)).copy()
        self.kp_lin, self.kd_lin, self.kp_ang, self.kd_ang = three(kp_lin), three(kd_lin), three(kp_ang), three(kd_ang)
        self.f_fb_max, self.t_fb_max, self.dev_max, self.tilt_max = float(f_fb_max), float(t_fb_max), float(dev_max), float(tilt_max)
        self.push_from, self.push_ticks = int(push_from), int(push_ticks)
        self.flags = FLAG_QUAT if quaternion else 0


def _vec(params, name, n, dtype):
    return [dtype(np.float64(v)) for v in np.array(getattr(params, name), np.float64).reshape(n)]


def plan_rows37(L, nodes, t0, hz, first_row, n_rows, dtype=np.longdouble):
    """The CSV rows first_row .. first_row + n_rows - 1 of the plan `nodes` [n_vars], [n_rows, 37] in dtype: qtos_sample_csv's
    columns (time stamp t0 + k / hz, the state at min(k / hz, T))."""
    off, t = plan_check.row_times(L, hz, first_row, n_rows)
    sp, x = L.splines, np.asarray(nodes, np.float64).reshape(-1)
    c = np.zeros((len(t), 37), dtype)
    c[:, 0] = dtype(np.float64(t0)) + off.astype(dtype)
    c[:, 1:4], c[:, 4:7] = plan_check.eval_spline(sp[0], x, t, 0, dtype), plan_check.eval_spline(sp[1], x, t, 0, dtype)
    c[:, 19:22], c[:, 22:25] = plan_check.eval_spline(sp[0], x, t, 1, dtype), plan_check.eval_spline(sp[1], x, t, 1, dtype)
    for e in range(NEE):
        c[:, 7 + 3 * e:10 + 3 * e] = plan_check.eval_spline(sp[2 + e], x, t, 0, dtype)
        c[:, 25 + 3 * e:28 + 3 * e] = plan_check.eval_spline(sp[6 + e], x, t, 0, dtype)
    return c


def plan_inputs(rows37, params=None, dtype=np.longdouble):
    """[n, 20] in dtype of CSV rows [n, 37]: the time stamp (0), r_p (1 .. 3), v_p (4 .. 6), q_p (7 .. 10), w_p (11 .. 13), F
    (14 .. 16) and tau_p (17 .. 19) of the module's docstring.  params: what ff_scale is read from (None: 1)."""
    c = np.asarray(rows37).astype(dtype).reshape(-1, 37)
    out = np.zeros((len(c), INPUTS), dtype)
    half = dtype(0.5)
    out[:, 0], out[:, 1:4], out[:, 4:7] = c[:, 0], c[:, 1:4], c[:, 19:22]
    sr, cr = np.sin(c[:, 4] * half), np.cos(c[:, 4] * half)
    sp, cp = np.sin(c[:, 5] * half), np.cos(c[:, 5] * half)
    sy, cy = np.sin(c[:, 6] * half), np.cos(c[:, 6] * half)
    out[:, 7] = sr * cp * cy - cr * sp * sy
    out[:, 8] = cr * sp * cy + sr * cp * sy
    out[:, 9] = cr * cp * sy - sr * sp * cy
    out[:, 10] = cr * cp * cy + sr * sp * sy
    sb, cb, sc, cc = np.sin(c[:, 5]), np.cos(c[:, 5]), np.sin(c[:, 6]), np.cos(c[:, 6])       # pitch, yaw
    out[:, 11] = cb * cc * c[:, 22] - sc * c[:, 23]
    out[:, 12] = cb * sc * c[:, 22] + cc * c[:, 23]
    out[:, 13] = c[:, 24] - sb * c[:, 22]
    ff = dtype(np.float64(1.0 if params is None else params.ff_scale))
    F = [None] * 3
    tau = [None] * 3
    for e in range(NEE):
        f = [c[:, 25 + 3 * e + i] for i in range(3)]
        d = [c[:, 7 + 3 * e + i] - c[:, 1 + i] for i in range(3)]
        x = [d[1] * f[2] - d[2] * f[1], d[2] * f[0] - d[0] * f[2], d[0] * f[1] - d[1] * f[0]]
        for i in range(3):
            F[i] = f[i] if e == 0 else F[i] + f[i]
            tau[i] = x[i] if e == 0 else tau[i] + x[i]
    for i in range(3):
        out[:, 14 + i], out[:, 17 + i] = ff * F[i], ff * tau[i]
    return out


def quat_matrix(q):
    """R (nine numbers, row-major) of the quaternion (x, y, z, w), from products of its components: tracking.quat_rotation's
    entries without the division by the norm."""
    x, y, z, w = q
    return [1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
            2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
            2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]


def _norm3(a):
    return np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])


def attitude_error(qp, q):
    """q_e = q_p (x) conj(q) as (x, y, z, w), negated if its w < 0."""
    px, py, pz, pw = qp
    x, y, z, w = q
    ex = ((pw * -x + px * w) + py * -z) - pz * -y
    ey = ((pw * -y - px * -z) + py * w) + pz * -x
    ez = ((pw * -z + px * -y) - py * -x) + pz * w
    ew = ((pw * w - px * -x) - py * -y) - pz * -z
    if ew < 0:
        ex, ey, ez, ew = -ex, -ey, -ez, -ew
    return [ex, ey, ez, ew]


def initial_state(row37, dtype=np.longdouble):
    """The state QTOS_ROLLOUT_INIT sets from a CSV row: r_p, v_p, q_p, R(q_p)^T w_p, [13] in dtype (the pose part of
    plan_inputs: F and tau_p are not read)."""
    p = plan_inputs(np.asarray(row37).reshape(1, 37), None, dtype)[0]
    s = np.zeros(STATE, dtype)
    s[0:3], s[3:6], s[6:10] = p[1:4], p[4:7], p[7:11]
    R, w = quat_matrix(p[7:11]), p[11:14]
    for i in range(3):
        s[10 + i] = (R[i] * w[0] + R[3 + i] * w[1]) + R[6 + i] * w[2]
    return s


def _clip(v, lim):
    """(clip(v, -lim, lim), whether it acted); lim <= 0: no clip.  A NaN stays a NaN."""
    if lim > 0:
        if v < -lim:
            return -lim, True
        if v > lim:
            return lim, True
    return v, False


def observe(state, inp):
    """(e [3], |e|, q_e [4], 2 |vec(q_e)|) of a state against a row of plan_inputs: lines 1, 5 of the step and columns 17, 18."""
    e = [state[i] - inp[1 + i] for i in range(3)]
    qe = attitude_error(inp[7:11], state[6:10])
    return e, _norm3(e), qe, 2 * _norm3(qe)


class Body:
    """The constants of a window's steps in dtype: the gains and limits, m_s = mass mass_scale, Ib_s = mass_scale inertia_b and
    Ib_s^-1 = inertia_b_inv / mass_scale, the push (zeros without one)."""

    def __init__(self, params, mass_scale=1.0, push=None, dtype=np.longdouble):
        d = dtype
        self.kpl, self.kdl, self.kpa, self.kda = (_vec(params, n, 3, d) for n in ("kp_lin", "kd_lin", "kp_ang", "kd_ang"))
        self.fmax, self.tmax = d(np.float64(params.f_fb_max)), d(np.float64(params.t_fb_max))
        ms = d(np.float64(mass_scale))
        self.m_s, self.g = d(np.float64(params.mass)) * ms, d(np.float64(params.gravity))
        self.Ib = [ms * x for x in _vec(params, "inertia_b", 9, d)]
        self.Ii = [x / ms for x in _vec(params, "inertia_b_inv", 9, d)]
        self.zero = [d(0)] * 3
        self.Fp = self.zero if push is None else [d(np.float64(x)) for x in np.asarray(push, np.float64).reshape(6)[0:3]]
        self.tp = self.zero if push is None else [d(np.float64(x)) for x in np.asarray(push, np.float64).reshape(6)[3:6]]


def step(state, inp, params, h, mass_scale=1.0, push=None, dtype=np.longdouble, body=None):
    """One step of length h (dtype) from `state` [13] under the row `inp` of plan_inputs: (new state, |F_fb|, whether a feedback
    component was clipped).  push: (F_push, tau_push) in the world, six numbers, or None.  body: a Body made once for many
    steps (then params, mass_scale and push are not read; the push acts iff `push` is not None)."""
    d = dtype
    M = Body(params, mass_scale, push, d) if body is None else body
    r, v, q, wb = list(state[0:3]), list(state[3:6]), list(state[6:10]), list(state[10:13])
    rp, vp, qp, wp, F, taup = inp[1:4], inp[4:7], inp[7:11], inp[11:14], inp[14:17], inp[17:20]
    kpl, kdl, kpa, kda, fmax, tmax, m_s, g, Ib, Ii = M.kpl, M.kdl, M.kpa, M.kda, M.fmax, M.tmax, M.m_s, M.g, M.Ib, M.Ii
    Fp, tp = (M.zero, M.zero) if push is None else (M.Fp, M.tp)
    clipped = False
    e = [r[i] - rp[i] for i in range(3)]                                                # 1
    fb = [None] * 3
    for i in range(3):                                                                  # 2
        fb[i], c = _clip(-(kpl[i] * e[i]) - kdl[i] * (v[i] - vp[i]), fmax)
        clipped = clipped or c
    a = [((F[i] + fb[i]) + Fp[i]) / m_s for i in range(3)]                              # 3
    a[2] = a[2] - g
    R = quat_matrix(q)                                                                  # 4
    qe = attitude_error(qp, q)                                                          # 5
    eR = [2 * qe[i] for i in range(3)]                                                  # 6
    tfb = [None] * 3
    for i in range(3):                                                                  # 7
        Rw = (R[3 * i] * wb[0] + R[3 * i + 1] * wb[1]) + R[3 * i + 2] * wb[2]
        tfb[i], c = _clip(kpa[i] * eR[i] + kda[i] * (wp[i] - Rw), tmax)
        clipped = clipped or c
    exF = [e[1] * F[2] - e[2] * F[1], e[2] * F[0] - e[0] * F[2], e[0] * F[1] - e[1] * F[0]]
    tau = [((taup[i] - exF[i]) + tfb[i]) + tp[i] for i in range(3)]                     # 8
    for i in range(3):                                                                  # 9
        v[i] = v[i] + h * a[i]
        r[i] = r[i] + h * v[i]
    tb = [(R[i] * tau[0] + R[3 + i] * tau[1]) + R[6 + i] * tau[2] for i in range(3)]    # 10: R^T tau
    Iw = [(Ib[3 * i] * wb[0] + Ib[3 * i + 1] * wb[1]) + Ib[3 * i + 2] * wb[2] for i in range(3)]
    gy = [wb[1] * Iw[2] - wb[2] * Iw[1], wb[2] * Iw[0] - wb[0] * Iw[2], wb[0] * Iw[1] - wb[1] * Iw[0]]
    n = [tb[i] - gy[i] for i in range(3)]
    wn = [wb[i] + h * ((Ii[3 * i] * n[0] + Ii[3 * i + 1] * n[1]) + Ii[3 * i + 2] * n[2]) for i in range(3)]
    x, y, z, w = q                                                                      # 11
    hh = h * d(0.5)
    dq = [(w * wn[0] + y * wn[2]) - z * wn[1], (w * wn[1] - x * wn[2]) + z * wn[0], (w * wn[2] + x * wn[1]) - y * wn[0],
          (-(x * wn[0]) - y * wn[1]) - z * wn[2]]
    qn = [q[i] + hh * dq[i] for i in range(4)]
    nn = np.sqrt(((qn[0] * qn[0] + qn[1] * qn[1]) + qn[2] * qn[2]) + qn[3] * qn[3])
    qn = [c / nn for c in qn]
    out = np.zeros(STATE, d)
    out[0:3], out[3:6], out[6:10], out[10:13] = r, v, qn, wn
    return out, _norm3(fb), clipped


def euler_of(q, dtype):
    """(roll, pitch, yaw, gimbal) from R(q) as tracking.measured_pose extracts them: atan2 / asin with the clip (by comparisons:
    a NaN stays a NaN)."""
    R = quat_matrix(q)
    one = dtype(1)
    s = -R[6]
    s = -one if s < -one else (one if s > one else s)
    return np.arctan2(R[7], R[8]), np.arcsin(s), np.arctan2(R[3], R[0]), bool(abs(R[6]) >= 1)


def rollout_rows(L, nodes, t0, hz, first_row, n_rows, params, state=None, count=0, word=0, mass_scale=1.0, push=None, joint=None,
                 init=None, dtype=np.longdouble):
    """The rows first_row .. first_row + n_rows - 1 of a window: (meas [n, 18 | 19], rows [n, 20], status [n] int32, state [13],
    count, word).  state / count / word: what the window carries (state None: QTOS_ROLLOUT_INIT, the state is set from row
    first_row of the plan; init=True forces that with a state given, and so does PENDING in `word`, which is cleared).  push: six numbers (F_push, tau_push), or None.  joint:
    joint rows [n, >= 13] whose columns 1 .. 12 become the measured joint angles (None: those twelve columns are 0 here; the
    kernel leaves them untouched -- the legs sit on their commands, and the foot error k_track then reports is the base error
    carried through the leg).  rows: the time stamp, r, the Euler angles, v, R w_b, q, |e|, 2 |vec(q_e)|, |F_fb| of the tick's
    first step."""
    d = dtype
    n = max(int(n_rows), 0)
    quat = bool(int(params.flags) & FLAG_QUAT)
    mcols = 19 if quat else 18
    meas, rows, status = np.zeros((n, mcols), d), np.zeros((n, ROW_COLS), d), np.zeros(n, np.int32)
    count, word = int(count), int(word)
    if n == 0:
        return meas, rows, status, (None if state is None else np.asarray(state).astype(d)), count, word
    with np.errstate(all="ignore"):
        c37 = plan_rows37(L, nodes, t0, hz, first_row, n, d)
        inputs = plan_inputs(c37, params, d)
        if state is None or init or word & PENDING:
            state = initial_state(c37[0], d)
        word &= ~PENDING
        state = np.asarray(state).astype(d)
        sub = int(params.substeps)
        h = d(1) / (d(np.float64(hz)) * d(sub))
        dev_max, tilt_max = d(np.float64(params.dev_max)), d(np.float64(params.tilt_max))
        body = Body(params, mass_scale, push, d)
        for j in range(n):
            inp = inputs[j]
            _, en, _, tilt = observe(state, inp)
            st = 0
            if not np.isfinite(state).all():
                word |= NONFINITE
            if (dev_max > 0 and en > dev_max) or (tilt_max > 0 and tilt > tilt_max):
                word |= FALLEN
            st |= word & (FALLEN | NONFINITE)
            roll, pitch, yaw, gimbal = euler_of(state[6:10], d)
            if gimbal:
                st |= GIMBAL
            R, wb = quat_matrix(state[6:10]), state[10:13]
            rows[j, 0], rows[j, 1:4], rows[j, 4:7], rows[j, 7:10] = inp[0], state[0:3], (roll, pitch, yaw), state[3:6]
            rows[j, 10:13] = [(R[3 * i] * wb[0] + R[3 * i + 1] * wb[1]) + R[3 * i + 2] * wb[2] for i in range(3)]
            rows[j, 13:17], rows[j, 17], rows[j, 18] = state[6:10], en, tilt
            meas[j, 0:3] = state[0:3]
            if quat:
                meas[j, 3:7] = state[6:10]
            else:
                meas[j, 3:6] = (roll, pitch, yaw)
            if joint is not None:
                meas[j, mcols - 12:] = np.asarray(joint)[j, 1:13]
            if not st & (FALLEN | NONFINITE):
                c = count + j
                acts = push is not None and int(params.push_from) <= c < int(params.push_from) + int(params.push_ticks)
                if acts:
                    st |= PUSH
                for s in range(sub):
                    state, fbn, clipped = step(state, inp, params, h, mass_scale, push if acts else None, d, body)
                    if s == 0:
                        rows[j, 19] = fbn
                    if clipped:
                        st |= CLIPPED
            status[j] = st
    return meas, rows, status, state, count + n, word
