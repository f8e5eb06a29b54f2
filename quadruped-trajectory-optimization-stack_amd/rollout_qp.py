"""Rollout with the force QP: the rollout's stance forces from the pyramid QP.  The rule of k_rollout_qp (qtos_rollout_qp*,
include/qtos_planner.h) stated in numpy, built from rollout_feet.py and force_qp.py, which it leaves as they are.

rollout_feet.py delivers the feedback wrench of every step through the stance feet and, with FEET_LIMIT, clips each force against
the vertical; force_qp.py minimises the fit's objective inside no-pulling, the friction pyramid and the force cap, on the plan's
own rows.  Here the second takes the place of the first's clip, in every step of the simulated closed loop.  A per-step optimum
is not a balance controller: the module reports what the limits cost the feedback, it cures nothing.

Everything is rollout_feet.rollout_feet_rows -- the inputs, the weights, lines 1 .. 11 of the step, the freeze, PENDING / INIT,
the columns of meas, rows and frows -- except the line that forms f_a.  Per step:

 1. f0_e = ff_scale f_e and df_e as rollout_feet.step forms them (M, y and d_e from the ACTUAL centre of mass).  With the basis
    force_qp.basis at slopes 0 (the rollout reads no terrain) the step takes the FIT PATH iff every stance foot's six limit values
    G (f0 + df) - h are <= 0, and then f_a = f0 + df: rollout_feet's unlimited step, to the bit.  A NaN fails the comparison, takes
    the limited path and runs into the step cap; the next row's freeze catches it.
 2. Otherwise (the LIMITED PATH) f_a = f0 + x, x = force_qp.solve_rows(d = d_e, w, stance, rho_s = rho~, c = damping n, slopes 0,
    f = f0, x_fit = df, mu, f_max, mu_end, max_iter): the central point at weight mu_end, strictly feasible, in the order of the
    operations that force_qp.py's docstring states.
 3. Swing feet and rows without a stance foot are rollout_feet's.

Parameters: FeetParams' fields (feet_flags is ignored) and mu_end, act_tol, max_iter; mu > 0 and f_max > 0 are required, as in
force_qp.QpParams.

Outputs: rollout_feet_rows' tuple with an 8-column table `qrows` of the tick's FIRST step behind frows, force_qp's QP_COLS:

   0   steps taken (0 on the fit path)
   1   max |s z - mu_end| / mu_end                       2   |r_d|inf                                   [N]
   3   the smallest slack over the stance feet  [N]      4   the largest multiplier
   5   sqrt(sum |x - df|^2)                     [N]      6   objective(x) - objective(df), >= 0         [N^2]
   7   the number of limit rows with slack <= act_tol

(on the fit path columns 0 .. 2 and 4 .. 6 are 0 and 3, 7 come from the fit's slacks; a row without stance and a frozen row have
zeros; columns 3 and 4 are taken by comparisons, which pass a NaN over, and a NaN slack is not counted in 7).  Status bits beside rollout_feet.py's: LIMITED (256) a step of this tick took the limited path, CAP (512) a step reached
max_iter.
"""
import numpy as np

from . import force_qp
from . import rollout as ro
from . import rollout_feet as rf

NEE = 4
FEET_COLS, QP_COLS = rf.FEET_COLS, force_qp.QP_COLS
NO_STANCE, TWO_STANCE, LIMITED, CAP = rf.NO_STANCE, rf.TWO_STANCE, rf.LIMITED, 512
MAX_ITER = force_qp.MAX_ITER


class QpFeetParams(rf.FeetParams):
    """FeetParams and the QP's: mu_end [N^2], act_tol [N], max_iter (1 .. 25).  capi.QtosRolloutQp has the same field names and is
    taken as well."""

    def __init__(self, cfg=None, arm=0.2, damping=1e-6, w_min=0.01, mu=None, f_max=None, mu_end=1e-6, act_tol=1e-3, max_iter=MAX_ITER):
        super().__init__(cfg, arm, damping, w_min, mu, f_max, False)
        self.mu_end, self.act_tol, self.max_iter = float(mu_end), float(act_tol), int(max_iter)
        check(self)


def check(feet):
    """ValueError unless the QP's parameters are in their ranges (force_qp.QpParams' conditions)."""
    if not feet.mu > 0 or not feet.f_max > 0 or not feet.mu_end > 0 or not (1 <= int(feet.max_iter) <= MAX_ITER) or feet.act_tol != feet.act_tol:
        raise ValueError("mu > 0, f_max > 0, mu_end > 0, max_iter in 1 .. 25, act_tol a number")


class _Unlimited:
    """The feet's fields as rollout_feet.step reads them, without its limit."""

    def __init__(self, feet):
        self.arm, self.damping, self.w_min, self.mu, self.f_max, self.feet_flags = feet.arm, feet.damping, feet.w_min, feet.mu, feet.f_max, 0


def _advance(state, inp, fa, lev, f0, fb, tfb, stance, h, body, push, dtype):
    """rollout_feet.step's lines behind f_a: (new state, miss_f, miss_t, change) from the applied forces fa [4][3], the levers, f0 =
    ff_scale f, the clipped feedback force and torque."""
    d = dtype
    B = body
    r, v, q, wb = list(state[0:3]), list(state[3:6]), list(state[6:10]), list(state[10:13])
    Fp, tp = (B.Fp, B.tp) if push else (B.zero, B.zero)
    R = ro.quat_matrix(q)
    Fa, ta = [None] * 3, [None] * 3
    gF, gT, sq = [d(0)] * 3, [d(0)] * 3, d(0)
    for k in range(NEE):
        x = rf._cross(lev[k], fa[k])
        for i in range(3):
            Fa[i] = fa[k][i] if k == 0 else Fa[i] + fa[k][i]
            ta[i] = x[i] if k == 0 else ta[i] + x[i]
        if stance[k]:
            g = [fa[k][i] - f0[k][i] for i in range(3)]
            x = rf._cross(lev[k], g)
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
    return new, ro._norm3(dF), ro._norm3(dT), np.sqrt(sq)


def _least(v, dtype, start=None):
    """The smallest of v taken by comparisons from `start` (None: +inf), as the kernel takes it: a NaN is never smaller, so it is
    passed over (all NaN: `start`)."""
    v = np.asarray(v, dtype).reshape(-1)
    with np.errstate(invalid="ignore"):
        v = v[v == v]
    return dtype(np.min(v, initial=dtype(np.inf) if start is None else start))


def step(state, inp, p, f, w, stance, feet, h, body, push, ff, dtype=np.longdouble, detail=False):
    """One step (rollout_feet.step's arguments; feet: a QpFeetParams or a QtosRolloutQp): (new state, |F_fb|, whether a feedback
    component was clipped, out).  out: rollout_feet.step's f_a, miss_f, miss_t, change, near (the feedback clips'), y, M, F_fb,
    tau_fb, lev, and limited, cap, steps, qcols [8], switch (the smallest |G (f0 + df) - h| over the stance feet, inf without
    stance), slack [4, 6] of the applied forces (NaN for a swing foot), f0, df, d [4, 3], rho [6], c, and on the limited path z
    [4, 6] and x [4, 3]; with `detail` also stop (the smallest |max(comp / CTOL, rd / its threshold) - 1| over the stop tests the
    iteration made; inf on the fit path)."""
    d = dtype
    new, fbn, clipped, out = rf.step(state, inp, p, f, w, stance, _Unlimited(feet), h, body, push, ff, d)
    stance = np.asarray(stance, bool)
    n = int(np.count_nonzero(stance))
    arm, mu, f_max = d(np.float64(feet.arm)), d(np.float64(feet.mu)), d(np.float64(feet.f_max))
    act_tol = d(np.float64(feet.act_tol))
    lev, y, tfb, fb = out["lev"], out["y"], out["tau_fb"], out["F_fb"]
    dd = np.array([[lev[k][i] / arm for i in range(3)] for k in range(NEE)], d)
    f0 = np.array([[ff * f[k][i] for i in range(3)] for k in range(NEE)], d)
    df = np.zeros((NEE, 3), d)
    for k in range(NEE):
        if stance[k]:
            x = rf._cross(y[0:3], dd[k])
            df[k] = [(x[i] + y[3 + i]) * w[k] for i in range(3)]
    rho = np.array([tfb[0] / arm, tfb[1] / arm, tfb[2] / arm, fb[0], fb[1], fb[2]], d)
    c = d(np.float64(feet.damping)) * d(n)
    Bs = force_qp.basis(np.zeros(1, d), np.zeros(1, d), d)
    hvec = np.zeros(6, d)
    hvec[1] = f_max
    val = np.full((NEE, 6), -np.inf, d)
    for k in range(NEE):
        if stance[k]:
            val[k] = force_qp.g_mul(Bs, mu, (f0[k] + df[k])[None])[0] - hvec
    inside = bool((np.where(stance[:, None], val, d(-1)) <= 0).all())
    switch = np.abs(np.where(stance[:, None], val, d(np.inf))).min() if n else d(np.inf)
    qcols = np.zeros(QP_COLS, d)
    slack = np.where(stance[:, None], -val, d(np.nan))
    out = dict(out, limited=False, cap=False, steps=0, switch=switch, f0=f0, df=df, d=dd, rho=rho, c=c, stop=d(np.inf))
    if n > 0 and not inside:
        st1 = stance[None]
        args = (dd[None], np.asarray(w, d)[None], st1, rho[None], np.array([c], d), np.zeros((1, NEE, 2), d), f0[None], df[None], feet.mu,
                feet.f_max, feet.mu_end)
        S = force_qp.solve_rows(*args, int(feet.max_iter), d)
        xs = np.where(stance[:, None], S["x"][0], d(0))
        fa = [[f0[k][i] + xs[k][i] if stance[k] else out["f_a"][k][i] for i in range(3)] for k in range(NEE)]
        new, miss_f, miss_t, change = _advance(state, inp, fa, lev, f0, fb, tfb, stance, h, body, push, d)
        dsq = d(0)
        for k in range(NEE):
            if stance[k]:
                e = xs[k] - df[k]
                dsq = dsq + ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
        gap = force_qp.objective_gap(args[0], args[1], st1, args[3], args[4], df[None], xs[None], d)[0]
        slack = np.where(stance[:, None], S["s"][0], d(np.nan))
        qcols[0] = d(int(S["steps"][0]))
        qcols[1], qcols[2] = S["comp"][0], S["rd"][0]
        qcols[3] = _least(S["s"][0][stance], d)
        qcols[4] = -_least(-S["z"][0][stance], d, d(0))
        qcols[5], qcols[6] = np.sqrt(dsq), gap
        out.update(f_a=np.array(fa, d), miss_f=miss_f, miss_t=miss_t, change=change, limited=True, cap=bool(S["cap"][0]),
                   steps=int(S["steps"][0]), z=S["z"][0], x=xs)
        if detail:                                   # the stop tests of the iterates 0 .. steps: the iteration cut short at each
            thr = d(np.float64(force_qp.RTOL)) * (d(1) + np.abs(S["q"][0]).max())
            tests = [(S["comp"][0], S["rd"][0])]
            for it in range(int(S["steps"][0])):
                T = force_qp.solve_rows(*args, it, d)
                tests.append((T["comp"][0], T["rd"][0]))
            out["stop"] = min(abs(max(cm / d(np.float64(force_qp.CTOL)), rd / thr) - d(1)) for cm, rd in tests)
    elif n > 0:
        qcols[3] = _least(slack[stance], d)
    with np.errstate(invalid="ignore"):
        qcols[7] = d(int(np.count_nonzero(stance[:, None] & (slack <= act_tol))))
    out["qcols"], out["slack"] = qcols, slack
    return new, fbn, clipped, out


def rollout_qp_rows(L, nodes, t0, hz, first_row, n_rows, params, feet=None, state=None, count=0, word=0, mass_scale=1.0, push=None,
                    joint=None, init=None, dtype=np.longdouble, detail=False, stop_tests=True):
    """The rows first_row .. first_row + n_rows - 1 of a window: (meas [n, 18 | 19], rows [n, 20], frows [n, 16], qrows [n, 8], status
    [n] int32, state [13], count, word).  The arguments are rollout_feet.rollout_feet_rows'; feet: a QpFeetParams (None: the
    defaults).  detail: also a dict, per row and over ALL steps of the tick -- switch, stop, near [n] (step's), steps [n, substeps]
    int, slack_min [n] (the smallest slack of an applied stance force; inf without stance or on a frozen row) -- and of the tick's
    FIRST step first [n] (step's `out`, None on a frozen row), and stance [n, 4], w [n, 4], alive [n] bool, enter [n, 13] the state
    the row starts from.  stop_tests False: `stop` is left at inf (it costs the iteration again, cut short at every iterate)."""
    d = dtype
    feet = QpFeetParams() if feet is None else feet
    check(feet)
    n = max(int(n_rows), 0)
    quat = bool(int(params.flags) & ro.FLAG_QUAT)
    mcols = 19 if quat else 18
    sub = int(params.substeps)
    meas, rows, frows, qrows = np.zeros((n, mcols), d), np.zeros((n, ro.ROW_COLS), d), np.zeros((n, FEET_COLS), d), np.zeros((n, QP_COLS), d)
    status = np.zeros(n, np.int32)
    count, word = int(count), int(word)
    det = dict(switch=np.full(n, np.inf, d), stop=np.full(n, np.inf, d), near=np.full(n, np.inf, d), steps=np.zeros((n, sub), np.int32),
               slack_min=np.full(n, np.inf, d), first=[None] * n, stance=np.zeros((n, NEE), bool), w=np.zeros((n, NEE), d),
               alive=np.zeros(n, bool), enter=np.zeros((n, ro.STATE), d))
    if n == 0:
        out = (meas, rows, frows, qrows, status, (None if state is None else np.asarray(state).astype(d)), count, word)
        return out + (det,) if detail else out
    with np.errstate(all="ignore"):
        c37 = ro.plan_rows37(L, nodes, t0, hz, first_row, n, d)
        inputs = ro.plan_inputs(c37, params, d)
        p, f, stance, w = rf.plan_feet(L, c37, hz, first_row, feet, d)
        det["stance"], det["w"] = stance, w
        if state is None or init or word & ro.PENDING:
            state = ro.initial_state(c37[0], d)
        word &= ~ro.PENDING
        state = np.asarray(state).astype(d)
        h = d(1) / (d(np.float64(hz)) * d(sub))
        ff = d(np.float64(params.ff_scale))
        dev_max, tilt_max = d(np.float64(params.dev_max)), d(np.float64(params.tilt_max))
        body = ro.Body(params, mass_scale, push, d)
        cnt = stance.sum(axis=1)
        for j in range(n):
            inp = inputs[j]
            det["enter"][j] = state
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
                det["alive"][j] = True
                c = count + j
                acts = push is not None and int(params.push_from) <= c < int(params.push_from) + int(params.push_ticks)
                if acts:
                    st |= ro.PUSH
                for s in range(sub):
                    state, fbn, clipped, out = step(state, inp, p[j], f[j], w[j], stance[j], feet, h, body, acts, ff, d, detail and stop_tests)
                    if s == 0:
                        rows[j, 19] = fbn
                        frows[j, 1:13], frows[j, 13], frows[j, 14], frows[j, 15] = out["f_a"].reshape(12), out["miss_f"], out["miss_t"], out["change"]
                        qrows[j] = out["qcols"]
                        det["first"][j] = out
                    det["near"][j], det["switch"][j] = min(det["near"][j], out["near"]), min(det["switch"][j], out["switch"])
                    det["stop"][j], det["steps"][j, s] = min(det["stop"][j], out["stop"]), out["steps"]
                    if cnt[j]:
                        det["slack_min"][j] = min(det["slack_min"][j], out["slack"][stance[j]].min())
                    if clipped:
                        st |= ro.CLIPPED
                    if out["limited"]:
                        st |= LIMITED
                    if out["cap"]:
                        st |= CAP
            status[j] = st
    out = (meas, rows, frows, qrows, status, state, count + n, word)
    return out + (det,) if detail else out
