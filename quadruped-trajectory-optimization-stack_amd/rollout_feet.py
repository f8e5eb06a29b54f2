"""Rollout through the feet: the rollout's feedback wrench delivered by the feet that stand.  The rule of k_rollout_feet
(qtos_rollout_feet*, include/qtos_planner.h) stated in numpy, built from rollout.py and force_fit.py, which it leaves as they are.

rollout.py applies its PD correction (F_fb, tau_fb) to the body as a free wrench.  A quadruped pushes only through the feet in
stance, and two point feet supply no moment about the line through them.  Here the feedback wrench of every step is distributed
over the stance feet by force_fit.py's damped, load-weighted 6 x 6 solve, the forces act at the plan's footholds about the ACTUAL
centre of mass, and with FEET_LIMIT every stance force is limited to what a foot can do: no pulling, a friction pyramid, a force
cap.  What the feet do not deliver is missing from the body's motion and reported per row.  It is still not a simulator of the
robot: no contacts (a foot pushes where the plan says it stands), no legs' inertia, no joint torques.

The number type is a parameter, as in rollout.py: dtype = np.longdouble is what the kernel is held to, np.float64 the same formulas
one rounded operation after the other.

Per row, in parallel: rollout.plan_inputs' 20 columns, and for every foot e in the order FL FR HL HR (plan_feet)

    p_e     the plan's foot position, CSV columns 7 + 3 e ..
    f_e     the plan's force, CSV columns 25 + 3 e ..
    stance  plan_check.stance_rows' flag: the motion polynomial is a stance (its rule for a row on a phase switch included)
    n       the number of stance feet
    w_e     the fit's load weights with g_e = f_e,z, the VERTICAL component of the plan's force:
            x = (n max(g_e, 0)) / sum_S max(g, 0), w_e = w_min where x < w_min, else x; all 1 where the sum is not > 0.
            force_fit.py takes g_e along the terrain normal under the foot; this rule takes the vertical -- the rollout reads no
            terrain -- and the two are equal on flat ground and on nearest-cell terrain (terrain_mode 1).

Per step (a tick takes `substeps` of them with the row held; every line is evaluated from the state at the step's start).  Lines
1, 2, 4 .. 7 and 9 .. 11 are rollout.step's, unchanged; its lines 3 and 8 are replaced:

    rho~    (tau_fb / arm, F_fb): the desired feedback wrench, the clipped PD terms of lines 7 and 2
    l_e     p_e - r, with r the STATE's position, not the plan's;  d_e = l_e / arm
    M       force_fit.system(d, w, stance, damping n);  y = force_fit.cholesky_solve(M, rho~), in that module's stated order;
            n = 0: y = 0 and nothing is delivered
    df_e    (cross(y[0:3], d_e) + y[3:6]) * w_e for a stance foot, force_fit.py's expression; 0 for a swing foot
    f_a,e   ff_scale f_e + df_e.  With FEET_LIMIT every STANCE foot's applied force is then limited by comparisons only (a NaN stays a
            NaN): z = f_z, 0 where f_z < 0; where f_max > 0, f_max where z > f_max; c = mu z; f_x and f_y each -c where below -c,
            c where above c.  The limit is against the vertical: the terrain normal only on flat and nearest-cell terrain.  Swing
            feet are not limited.
    F_a     ((f_a,0 + f_a,1) + f_a,2) + f_a,3;  tau_a the sum, in the same foot order, of l_e x f_a,e
     3      a = (F_a + F_push) / m_s - g e_z
     8      tau = tau_a + tau_push   (rollout.py's term -e x F is inside tau_a: the levers are taken from the actual CoM)

With all gains 0, ff_scale 1 and no limit df = 0 exactly, and r, v are rollout.py's to the bit.

Outputs per row: meas, the 20-column rows and state / count / word exactly as rollout.rollout_rows gives them (column 19 stays
|F_fb|, the DESIRED feedback force of the tick's first step; the sticky fallen / non-finite freeze, PENDING and INIT likewise), and
a second table `frows` of 16 columns (FEET_COLS), with g_e = f_a,e - ff_scale f_e of the tick's first step:

    0          the time stamp
    1 .. 12    f_a of the tick's first step                                                                    [N]
    13         |sum_S g_e - F_fb|, the sum foot after foot from 0, |.| = sqrt((x x + y y) + z z)               [N]
    14         |sum_S l_e x g_e - tau_fb|                                                                      [N m]
    15         sqrt(sum_S |g_e|^2)                                                                             [N]

Columns 13 and 14 are what the feet did not deliver.  A frozen row has 0 in columns 13 .. 15 and the plan's forces f_e in 1 .. 12.
Status bits beside rollout.py's: NO_STANCE (64) no stance foot in this row, TWO_STANCE (128) exactly two, LIMITED (256) a
comparison of the limit acted in a step of this tick (never on a frozen row).
"""
import numpy as np

from . import force_fit
from . import plan_check
from . import rollout as ro

NEE = 4
FEET_COLS = 16
FEET_LIMIT = 1                                  # QtosRolloutFeet.feet_flags: QTOS_FEET_LIMIT
NO_STANCE, TWO_STANCE, LIMITED = 64, 128, 256   # status bits of a row, beside rollout.py's (PENDING is 32)


class FeetParams:
    """What the rule reads beside a RolloutParams.  capi.QtosRolloutFeet has the same field names and is taken as well.  arm,
    damping and w_min default to the fit's (force_fit.FitParams); mu and f_max to the planner configuration's friction and force
    limit (cfg None: PlannerConfig's defaults)."""

    def __init__(self, cfg=None, arm=0.2, damping=1e-6, w_min=0.01, mu=None, f_max=None, limit=False):
        if cfg is None:
            from .config import PlannerConfig
            cfg = PlannerConfig()
        self.arm, self.damping, self.w_min = float(arm), float(damping), float(w_min)
        self.mu = float(cfg.friction if mu is None else mu)
        self.f_max = float(cfg.force_limit if f_max is None else f_max)
        if not self.arm > 0 or not self.damping > 0 or not (0 < self.w_min <= 1) or not self.mu >= 0:
            raise ValueError("arm > 0, damping > 0, 0 < w_min <= 1 and mu >= 0")
        self.feet_flags = FEET_LIMIT if limit else 0


def plan_feet(L, rows37, hz, first_row, feet, dtype=np.longdouble):
    """(p [n, 4, 3], f [n, 4, 3], stance [n, 4] bool, w [n, 4]) of the CSV rows [n, 37] first_row .. of a plan: the per-row part of
    the module's docstring."""
    c = np.asarray(rows37).astype(dtype).reshape(-1, 37)
    n = len(c)
    p, f = c[:, 7:19].reshape(n, NEE, 3).copy(), c[:, 25:37].reshape(n, NEE, 3).copy()
    stance = plan_check.stance_rows(L, hz, first_row, n)
    nn = stance.sum(axis=1).astype(dtype)
    w_min = dtype(np.float64(feet.w_min))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        g = f[:, :, 2]
        gpos = np.where(stance & (g > 0), g, dtype(0))
        gsum = ((gpos[:, 0] + gpos[:, 1]) + gpos[:, 2]) + gpos[:, 3]
        loaded = gsum > 0
        x = (nn[:, None] * gpos) / np.where(loaded, gsum, dtype(1))[:, None]
        w = np.where(loaded[:, None], np.where(x < w_min, w_min, x), dtype(1))
    return p, f, stance, w


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _limit(f, mu, f_max, zero):
    """The limit of one stance force, by comparisons only: ([x, y, z], whether a comparison acted, the smallest distance of a
    compared value from its threshold).  zero: 0 in the number type."""
    x, y, z = f
    acted = False
    near = abs(z)
    if f_max > 0:
        near = min(near, abs(z - f_max))
    c = mu * (f_max if f_max > 0 and z > f_max else (zero if z < 0 else z))
    near = min(near, abs(x + c), abs(x - c), abs(y + c), abs(y - c))
    if z < 0:
        z, acted = zero, True
    if f_max > 0 and z > f_max:
        z, acted = f_max, True
    c = mu * z
    if x < -c:
        x, acted = -c, True
    elif x > c:
        x, acted = c, True
    if y < -c:
        y, acted = -c, True
    elif y > c:
        y, acted = c, True
    return [x, y, z], acted, near


def step(state, inp, p, f, w, stance, feet, h, body, push, ff, dtype=np.longdouble):
    """One step of length h (dtype) from `state` [13] under the row `inp` of rollout.plan_inputs with the feet p, f [4, 3], w [4]
    and stance [4] of plan_feet: (new state, |F_fb|, whether a feedback component was clipped, out).  body: a rollout.Body; the push
    acts iff `push`; ff: ff_scale in dtype.  out: f_a [4, 3], dF and dT [3] (the signed vectors behind columns 13 and 14), miss_f,
    miss_t, change (columns 13 .. 15), limited, near (the smallest distance of a compared value -- of a feedback clip or of the
    limit -- from its threshold; inf without either), y [6] and M [6, 6]."""
    d = dtype
    B = body
    r, v, q, wb = list(state[0:3]), list(state[3:6]), list(state[6:10]), list(state[10:13])
    rp, vp, qp, wp = inp[1:4], inp[4:7], inp[7:11], inp[11:14]
    Fp, tp = (B.Fp, B.tp) if push else (B.zero, B.zero)
    clipped = False
    e = [r[i] - rp[i] for i in range(3)]                                                # 1
    fb, fb_raw, tfb_raw = [None] * 3, [None] * 3, [None] * 3
    for i in range(3):                                                                  # 2
        fb_raw[i] = -(B.kpl[i] * e[i]) - B.kdl[i] * (v[i] - vp[i])
        fb[i], c = ro._clip(fb_raw[i], B.fmax)
        clipped = clipped or c
    R = ro.quat_matrix(q)                                                               # 4
    qe = ro.attitude_error(qp, q)                                                       # 5
    eR = [2 * qe[i] for i in range(3)]                                                  # 6
    tfb = [None] * 3
    for i in range(3):                                                                  # 7
        Rw = (R[3 * i] * wb[0] + R[3 * i + 1] * wb[1]) + R[3 * i + 2] * wb[2]
        tfb_raw[i] = B.kpa[i] * eR[i] + B.kda[i] * (wp[i] - Rw)
        tfb[i], c = ro._clip(tfb_raw[i], B.tmax)
        clipped = clipped or c
    # the feedback wrench through the stance feet
    arm, mu, f_max = d(np.float64(feet.arm)), d(np.float64(feet.mu)), d(np.float64(feet.f_max))
    rho = np.array([tfb[0] / arm, tfb[1] / arm, tfb[2] / arm, fb[0], fb[1], fb[2]], d)
    lev = [[p[k][i] - r[i] for i in range(3)] for k in range(NEE)]
    dd = np.array([[lev[k][i] / arm for i in range(3)] for k in range(NEE)], d)
    n = int(np.count_nonzero(stance))
    lam = d(np.float64(feet.damping)) * d(n)
    M = force_fit.system(dd[None], np.asarray(w, d)[None], np.asarray(stance, bool)[None], np.array([lam], d), d)
    y = force_fit.cholesky_solve(M, rho[None], d)[0] if n > 0 else np.zeros(6, d)
    fa, limited, near = [None] * NEE, False, d(np.inf)
    for lim, vals in ((B.fmax, fb_raw), (B.tmax, tfb_raw)):      # (the feedback clips' thresholds)
        if lim > 0:
            near = min([near] + [min(abs(x - lim), abs(x + lim)) for x in vals])
    for k in range(NEE):
        df = [d(0)] * 3
        if stance[k]:
            x = _cross(y[0:3], dd[k])
            df = [(x[i] + y[3 + i]) * w[k] for i in range(3)]
        fa[k] = [ff * f[k][i] + df[i] for i in range(3)]
        if stance[k] and int(feet.feet_flags) & FEET_LIMIT:
            fa[k], c, m = _limit(fa[k], mu, f_max, d(0))
            limited, near = limited or c, min(near, m)
    Fa, ta = [None] * 3, [None] * 3
    gF, gT, sq = [d(0)] * 3, [d(0)] * 3, d(0)
    for k in range(NEE):
        x = _cross(lev[k], fa[k])
        for i in range(3):
            Fa[i] = fa[k][i] if k == 0 else Fa[i] + fa[k][i]
            ta[i] = x[i] if k == 0 else ta[i] + x[i]
        if stance[k]:
            g = [fa[k][i] - ff * f[k][i] for i in range(3)]
            x = _cross(lev[k], g)
            for i in range(3):
                gF[i], gT[i] = gF[i] + g[i], gT[i] + x[i]
            sq = sq + ((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    dF, dT = [gF[i] - fb[i] for i in range(3)], [gT[i] - tfb[i] for i in range(3)]
    a = [(Fa[i] + Fp[i]) / B.m_s for i in range(3)]                                     # 3
    a[2] = a[2] - B.g
    tau = [ta[i] + tp[i] for i in range(3)]                                             # 8
    for i in range(3):                                                                  # 9
        v[i] = v[i] + h * a[i]
        r[i] = r[i] + h * v[i]
    Ib, Ii = B.Ib, B.Ii
    tb = [(R[i] * tau[0] + R[3 + i] * tau[1]) + R[6 + i] * tau[2] for i in range(3)]    # 10: R^T tau
    Iw = [(Ib[3 * i] * wb[0] + Ib[3 * i + 1] * wb[1]) + Ib[3 * i + 2] * wb[2] for i in range(3)]
    gy = [wb[1] * Iw[2] - wb[2] * Iw[1], wb[2] * Iw[0] - wb[0] * Iw[2], wb[0] * Iw[1] - wb[1] * Iw[0]]
    nt = [tb[i] - gy[i] for i in range(3)]
    wn = [wb[i] + h * ((Ii[3 * i] * nt[0] + Ii[3 * i + 1] * nt[1]) + Ii[3 * i + 2] * nt[2]) for i in range(3)]
    x, yq, z, wq = q                                                                    # 11
    hh = h * d(0.5)
    dq = [(wq * wn[0] + yq * wn[2]) - z * wn[1], (wq * wn[1] - x * wn[2]) + z * wn[0], (wq * wn[2] + x * wn[1]) - yq * wn[0],
          (-(x * wn[0]) - yq * wn[1]) - z * wn[2]]
    qn = [q[i] + hh * dq[i] for i in range(4)]
    nn = np.sqrt(((qn[0] * qn[0] + qn[1] * qn[1]) + qn[2] * qn[2]) + qn[3] * qn[3])
    qn = [c / nn for c in qn]
    new = np.zeros(ro.STATE, d)
    new[0:3], new[3:6], new[6:10], new[10:13] = r, v, qn, wn
    out = dict(f_a=np.array(fa, d), dF=np.array(dF, d), dT=np.array(dT, d), miss_f=ro._norm3(dF), miss_t=ro._norm3(dT), change=np.sqrt(sq),
               limited=limited, near=near, y=y, M=M[0], tau_fb=np.array(tfb, d), F_fb=np.array(fb, d), lev=np.array(lev, d))
    return new, ro._norm3(fb), clipped, out


def rollout_feet_rows(L, nodes, t0, hz, first_row, n_rows, params, feet=None, state=None, count=0, word=0, mass_scale=1.0, push=None,
                      joint=None, init=None, dtype=np.longdouble, detail=False):
    """The rows first_row .. first_row + n_rows - 1 of a window: (meas [n, 18 | 19], rows [n, 20], frows [n, 16], status [n] int32,
    state [13], count, word).  params: a rollout.RolloutParams (or a QtosRollout); feet: a FeetParams (None: the defaults); every
    other argument is rollout.rollout_rows'.  detail: also a dict of the first step of every row -- y [n, 6], M [n, 6, 6], dF, dT,
    F_fb, tau_fb [n, 3], lev [n, 4, 3] (zeros on frozen rows), near [n] (over all steps of the tick: step's `near`), and stance
    [n, 4], w [n, 4]."""
    d = dtype
    feet = FeetParams() if feet is None else feet
    n = max(int(n_rows), 0)
    quat = bool(int(params.flags) & ro.FLAG_QUAT)
    mcols = 19 if quat else 18
    meas, rows, frows = np.zeros((n, mcols), d), np.zeros((n, ro.ROW_COLS), d), np.zeros((n, FEET_COLS), d)
    status = np.zeros(n, np.int32)
    count, word = int(count), int(word)
    det = dict(y=np.zeros((n, 6), d), M=np.zeros((n, 6, 6), d), dF=np.zeros((n, 3), d), dT=np.zeros((n, 3), d), F_fb=np.zeros((n, 3), d),
               tau_fb=np.zeros((n, 3), d), lev=np.zeros((n, NEE, 3), d), near=np.full(n, np.inf, d), stance=np.zeros((n, NEE), bool), w=np.zeros((n, NEE), d))
    if n == 0:
        out = (meas, rows, frows, status, (None if state is None else np.asarray(state).astype(d)), count, word)
        return out + (det,) if detail else out
    with np.errstate(all="ignore"):
        c37 = ro.plan_rows37(L, nodes, t0, hz, first_row, n, d)
        inputs = ro.plan_inputs(c37, params, d)
        p, f, stance, w = plan_feet(L, c37, hz, first_row, feet, d)
        det["stance"], det["w"] = stance, w
        if state is None or init or word & ro.PENDING:
            state = ro.initial_state(c37[0], d)
        word &= ~ro.PENDING
        state = np.asarray(state).astype(d)
        sub = int(params.substeps)
        h = d(1) / (d(np.float64(hz)) * d(sub))
        ff = d(np.float64(params.ff_scale))
        dev_max, tilt_max = d(np.float64(params.dev_max)), d(np.float64(params.tilt_max))
        body = ro.Body(params, mass_scale, push, d)
        cnt = stance.sum(axis=1)
        for j in range(n):
            inp = inputs[j]
            _, en, _, tilt = ro.observe(state, inp)
            st = 0
            if not np.isfinite(state).all():
                word |= ro.NONFINITE
            if (dev_max > 0 and en > dev_max) or (tilt_max > 0 and tilt > tilt_max):
                word |= ro.FALLEN
            st |= word & (ro.FALLEN | ro.NONFINITE)
            roll, pitch, yaw, gimbal = ro.euler_of(state[6:10], d)
            if gimbal:
                st |= ro.GIMBAL
            st |= (NO_STANCE if cnt[j] == 0 else 0) | (TWO_STANCE if cnt[j] == 2 else 0)
            R, wb = ro.quat_matrix(state[6:10]), state[10:13]
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
            frows[j, 0], frows[j, 1:13] = inp[0], f[j].reshape(12)
            if not st & (ro.FALLEN | ro.NONFINITE):
                c = count + j
                acts = push is not None and int(params.push_from) <= c < int(params.push_from) + int(params.push_ticks)
                if acts:
                    st |= ro.PUSH
                for s in range(sub):
                    state, fbn, clipped, out = step(state, inp, p[j], f[j], w[j], stance[j], feet, h, body, acts, ff, d)
                    if s == 0:
                        rows[j, 19] = fbn
                        frows[j, 1:13], frows[j, 13], frows[j, 14], frows[j, 15] = out["f_a"].reshape(12), out["miss_f"], out["miss_t"], out["change"]
                        for key in ("y", "M", "dF", "dT", "F_fb", "tau_fb", "lev"):
                            det[key][j] = out[key]
                    det["near"][j] = min(det["near"][j], out["near"])
                    if clipped:
                        st |= ro.CLIPPED
                    if out["limited"]:
                        st |= LIMITED
            status[j] = st
    out = (meas, rows, frows, status, state, count + n, word)
    return out + (det,) if detail else out
