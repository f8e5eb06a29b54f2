"""The interior-point iteration around the KKT solve, restated in plain numpy (TEST INFRASTRUCTURE ONLY).

What k_start and k_step (csrc/kernels.hpp) do around the splines, the linearisation and the KKT solve -- the slack push and
the first mu, the barrier weights, the slack and multiplier steps, the two fraction-to-the-boundary ratio tests, the Armijo
backtracking on the l1 infeasibility, the update with the clip of z, the mu rule, the measures and the chord / hold / stall /
jam decisions -- stated from DESIGN.md section 4 and the comments of config.py, one small function per thing the tests compare
(tests/test_step_cpu.py against the C oracle's whole solves, tests/test_gpu_steps.py against every single step of the kernels).

The per-row functions work elementwise on arrays of INEQUALITY rows (the caller slices g, s, z, lo, hi with the row list);
start_state takes all rows and the row kinds.  A bound below -1e19 / above 1e19 is no bound.  float64 throughout, np.longdouble
where a sum or a quotient is compared at rounding level.  The oracle's constraints / jacobian are the only model code used.
"""
import numpy as np

NO_BOUND = 1e19
KAPPA = 1e10                 # z stays within [mu / (kappa gap), kappa mu / gap]: the default of cfg.kappa_sigma (Ipopt's kappa_sigma)
ARMIJO = 1e-4
MAX_TRIALS = 6
TH_FLOOR = 1e-9              # an l1 infeasibility below this is accepted whatever it was before
MU_STEP = 0.3                # mu goes down behind a step longer than this
NEE = 4


def has_bounds(lo, hi):
    return lo > -NO_BOUND, hi < NO_BOUND


# ---- working set -----------------------------------------------------------------------------------------------------
def working_set(O, q, seed=1):
    """(free, E, I, lo, hi, row_kind): the free variables (bounds differ), the equality rows of the working set, the
    inequality rows, the row bounds and the kind per row (0 left out, 1 equality, 2 inequality).  An equality row is left out
    when no free variable enters it, or when it repeats an earlier equality row (the time grid ends with T twice where T is a
    whole number of steps: the second copy of the dynamics block is the same six equations).  Found on the Jacobian at a
    seeded generic point, rows compared entry by entry to 1e-9."""
    xl, xh = O.var_bounds(q)
    lo, hi = O.con_bounds()
    free = np.nonzero(xl != xh)[0]
    x = O.initial_guess(q) + 1e-2 * (np.random.default_rng(seed).random(O.n) - 0.5)
    J = O.jacobian(x)[:, free]
    kind = np.zeros(O.m, np.int32)
    kind[lo != hi] = 2
    seen = {}
    nd = O.L.n_dyn_times
    twice = nd >= 2 and abs(O.L.T - (nd - 2) * O.p.dt_dyn) < 1e-9          # the dynamics grid 0, dt, 2 dt, ... and then T
    for r in np.nonzero(lo == hi)[0]:
        cols = np.nonzero(J[r])[0]
        if not len(cols) or (twice and O.L.off_dyn + 6 * (nd - 1) <= r < O.L.off_dyn + 6 * nd):
            continue
        key = tuple(cols)
        if any(np.all(np.abs(J[r, cols] - J[r2, cols]) <= 1e-9 * (1 + np.abs(J[r, cols]))) for r2 in seen.get(key, ())):
            continue
        seen.setdefault(key, []).append(r)
        kind[r] = 1
    return free, np.nonzero(kind == 1)[0], np.nonzero(kind == 2)[0], lo, hi, kind


def stance_foothold_vars(O, cfg):
    """x and y of every stance foothold: a foot's motion variables are 3 per stance and 5 per swing, in phase order."""
    out = []
    for e in range(NEE):
        for sn in range((len(cfg.phase_durations[e]) + 1) // 2):
            out += [O.L.off_eem[e] + 8 * sn, O.L.off_eem[e] + 8 * sn + 1]
    return np.array(out)


# ---- the pieces ------------------------------------------------------------------------------------------------------
def measures(g, s, zl, zu, lo, hi, g_eq=()):
    """(viol, theta, compl): the largest bound violation of the working rows, the largest residual of the slack form
    (c_E, c_I - s) and the largest |gap x z|.  g, s, z, lo, hi: the inequality rows; g_eq: the equality rows' values."""
    hl, hu = has_bounds(lo, hi)
    eq = float(np.abs(g_eq).max()) if len(g_eq) else 0.0
    viol = max(eq, float(np.maximum(lo - g, g - hi).max()) if len(g) else 0.0)
    theta = max(eq, float(np.abs(g - s).max()) if len(g) else 0.0)
    compl = max(float(np.abs(np.where(hl, (s - lo) * zl, 0.0)).max()), float(np.abs(np.where(hu, (hi - s) * zu, 0.0)).max())) if len(g) else 0.0
    return viol, theta, compl


def start_state(g0, lo, hi, row_kind, cfg, warm):
    """(s, zl, zu, mu, viol, theta) of a starting point with constraint values g0 (all rows; s, z zero off the inequality
    rows).  The slack is g pushed inside its bounds by push x max(1, |bound|), on a two-sided row by no more than push x the
    range; push = slack_push on a cold start, warm_slack_push for given nodes or a table start.  mu0 = max(mu_min,
    min(mu_init, 0.01 theta^2)), z = mu / gap."""
    I, E = row_kind == 2, row_kind == 1
    hl, hu = has_bounds(lo, hi)
    kp = cfg.warm_slack_push if warm else cfg.slack_push
    pl = np.where(hl, kp * np.maximum(1.0, np.abs(lo)), 0.0)
    pu = np.where(hu, kp * np.maximum(1.0, np.abs(hi)), 0.0)
    both = hl & hu
    rng = np.where(both, hi - lo, 0.0)
    pl = np.where(both, np.minimum(pl, kp * rng), pl)
    pu = np.where(both, np.minimum(pu, kp * rng), pu)
    s = g0.copy()
    s = np.where(hl, np.maximum(s, np.where(hl, lo, 0.0) + pl), s)
    s = np.where(hu, np.minimum(s, np.where(hu, hi, 0.0) - pu), s)
    s = np.where(I, s, 0.0)
    viol, theta, _ = measures(g0[I], s[I], 0, 0, lo[I], hi[I], g0[E])
    mu = first_mu(theta, cfg)
    zl = np.where(I & hl, mu / np.where(I & hl, s - lo, 1.0), 0.0)
    zu = np.where(I & hu, mu / np.where(I & hu, hi - s, 1.0), 0.0)
    return s, zl, zu, mu, viol, theta


def first_mu(theta, cfg):
    return max(cfg.mu_min, min(cfg.mu_init, 0.01 * theta * theta))


def gaps(s, lo, hi):
    """(hl, hu, s - lo, hi - s) with 1 where there is no bound."""
    hl, hu = has_bounds(lo, hi)
    return hl, hu, np.where(hl, s - np.where(hl, lo, 0.0), 1.0), np.where(hu, np.where(hu, hi, 0.0) - s, 1.0)


def barrier_terms(g, s, zl, zu, mu, lo, hi):
    """(sig, w): the barrier's weight of a row, z_l / (s - l) + z_u / (u - s), and its right-hand side
    sig (g - s) - mu / (s - l) + mu / (u - s)."""
    hl, hu, dl, du = gaps(s, lo, hi)
    sig = np.where(hl, zl / dl, 0.0) + np.where(hu, zu / du, 0.0)
    gmu = -np.where(hl, mu / dl, 0.0) + np.where(hu, mu / du, 0.0)
    return sig, sig * (g - s) + gmu


def kkt_matrix(J, free, E, I, sig, diag, eps_rows):
    """[[diag + J_I' Sig J_I, J_E'], [J_E, -eps]] over (free variables, equality rows); sig by constraint row."""
    JE, JI = J[np.ix_(E, free)], J[np.ix_(I, free)]
    nf, nE = len(free), len(E)
    K = np.zeros((nf + nE, nf + nE))
    K[:nf, :nf] = np.diag(np.broadcast_to(np.asarray(diag, float), (nf,))) + JI.T @ (sig[I][:, None] * JI)
    K[nf:, :nf] = JE
    K[:nf, nf:] = JE.T
    K[nf:, nf:] = -np.diag(eps_rows)
    return K


def kkt_rhs(J, g, free, E, I, w):
    return np.concatenate([-J[np.ix_(I, free)].T @ w[I], -g[E]])


def solve_refined(K, rhs, lu=None):
    """LAPACK's solution of K h = rhs refined with residuals in extended precision.  Returns (h, the last refinement's
    largest correction, the factorisation)."""
    from scipy.linalg import lu_factor, lu_solve
    lu = lu_factor(K) if lu is None else lu
    Kl, bl = K.astype(np.longdouble), rhs.astype(np.longdouble)
    hp = lu_solve(lu, rhs).astype(np.longdouble)
    for _ in range(4):
        corr = lu_solve(lu, (bl - Kl @ hp).astype(np.float64))
        hp = hp + corr.astype(np.longdouble)
    return hp, corr, lu


def direction(J, g, free, E, I, sig, w, diag, eps_rows):
    """The Newton step of the free variables: the dense KKT system of the Jacobian J (all rows and columns), the constraint
    values g and the barrier terms sig, w (by constraint row), diag on the variables' diagonal (delta_x; the hold weight on
    the held footholds) and eps_rows on the multipliers'.  Returns (step, the last refinement's largest correction relative
    to the step's largest entry: what the dense solve itself may still be off by)."""
    hp, corr, _ = solve_refined(kkt_matrix(J, free, E, I, sig, diag, eps_rows), kkt_rhs(J, g, free, E, I, w))
    nf = len(free)
    return hp[:nf].astype(np.float64), float(np.abs(corr[:nf]).max() / np.abs(hp[:nf]).max())


def chord_direction(K_factored, J_new, g_new, w_new, free, E, I, lu=None):
    """A chord step: the matrix of the iterate that was factored, the right-hand side of the new one."""
    hp, corr, _ = solve_refined(K_factored, kkt_rhs(J_new, g_new, free, E, I, w_new), lu)
    nf = len(free)
    return hp[:nf].astype(np.float64), float(np.abs(corr[:nf]).max() / np.abs(hp[:nf]).max())


def slack_and_dual_steps(J_I, dx, g, s, zl, zu, mu, lo, hi):
    """(ds, dzl, dzu): ds = J_I dx + (g - s); dz_l = mu / (s - l) - z_l - z_l / (s - l) ds, dz_u = mu / (u - s) - z_u +
    z_u / (u - s) ds."""
    ds = (J_I.astype(np.longdouble) @ dx.astype(np.longdouble)).astype(np.float64) + (g - s)
    return (ds,) + dual_steps(s, ds, zl, zu, mu, lo, hi)


def dual_steps(s, ds, zl, zu, mu, lo, hi):
    hl, hu, dl, du = gaps(s, lo, hi)
    return np.where(hl, mu / dl - zl - zl / dl * ds, 0.0), np.where(hu, mu / du - zu + zu / du * ds, 0.0)


def step_lengths(s, ds, zl, zu, dzl, dzu, mu, lo, hi):
    """(amax, az): the longest steps <= 1 that keep the fraction 1 - tau of every gap and of every multiplier,
    tau = max(0.99, 1 - mu)."""
    tau = max(0.99, 1.0 - mu)
    hl, hu, dl, du = gaps(s, lo, hi)
    amax = az = 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        for on, num, den in ((hl & (ds < 0), dl, -ds), (hu & (ds > 0), du, ds)):
            if on.any():
                amax = min(amax, float((tau * num[on] / den[on]).min()))
        for on, num, den in ((hl & (dzl < 0), zl, -dzl), (hu & (dzu < 0), zu, -dzu)):
            if on.any():
                az = min(az, float((tau * num[on] / den[on]).min()))
    return amax, az


def l1_infeasibility(g, s, E, I):
    """Sum over the working rows of |c_E|, |c_I - s| (s by inequality row), in extended precision."""
    return float(np.abs(g[E].astype(np.longdouble)).sum() + np.abs(g[I].astype(np.longdouble) - s.astype(np.longdouble)).sum())


def line_search(constraints, x, dx, s, ds, amax, rows):
    """Backtracking from amax on the l1 infeasibility th of (c_E, c_I - s): a trial alpha is accepted when
    th(alpha) <= (1 - 1e-4 alpha) th(0) or th(alpha) < 1e-9, else halved; the sixth trial is taken as it is.  rows = (E, I);
    s, ds by inequality row.  Returns (alpha, trials, per trial a dict alpha, th, rhs, margin = th - rhs, accepted)."""
    E, I = rows
    th0 = l1_infeasibility(constraints(x), s, E, I)
    al, log = amax, []
    for t in range(MAX_TRIALS):
        th = l1_infeasibility(constraints(x + al * dx), s + al * ds, E, I)
        rhs = (1.0 - ARMIJO * al) * th0
        ok = th <= rhs or th < TH_FLOOR
        log.append(dict(alpha=al, th=th, rhs=rhs, margin=th - rhs, accepted=bool(ok), th0=th0))
        if ok or t == MAX_TRIALS - 1:
            break
        al *= 0.5
    return al, len(log), log


def kappa_of(cfg):
    return KAPPA if cfg is None else float(cfg.kappa_sigma)


def clip_limits(s_new, mu, lo, hi, cfg=None):
    """(lowest z_l, highest z_l, lowest z_u, highest z_u) of update(): mu / (kappa gap), kappa mu / gap at the NEW gap and the
    OLD mu, kappa = cfg.kappa_sigma."""
    kap = kappa_of(cfg)
    _, _, dl, du = gaps(s_new, lo, hi)
    return mu / (kap * dl), kap * mu / dl, mu / (kap * du), kap * mu / du


def update(s, ds, zl, zu, dzl, dzu, alpha, az, mu, lo, hi, cfg=None):
    """New (s, zl, zu): s + alpha ds, z + az dz clipped to [mu / (kappa gap), kappa mu / gap] at the NEW gap and the OLD mu."""
    sn = s + alpha * ds
    hl, hu = has_bounds(lo, hi)
    a, c = zl + az * dzl, zu + az * dzu
    lo_l, hi_l, lo_u, hi_u = clip_limits(sn, mu, lo, hi, cfg)
    a = np.where(hl, np.minimum(np.maximum(a, lo_l), hi_l), a)
    c = np.where(hu, np.minimum(np.maximum(c, lo_u), hi_u), c)
    return sn, a, c


def clip_sides(s_new, zl, zu, dzl, dzu, az, mu, lo, hi, cfg=None):
    """Per row, which limit of update() acts: (z_l at its lowest, z_l at its highest, z_u at its lowest, z_u at its highest)."""
    hl, hu = has_bounds(lo, hi)
    a, c = zl + az * dzl, zu + az * dzu
    lo_l, hi_l, lo_u, hi_u = clip_limits(s_new, mu, lo, hi, cfg)
    return hl & (a < lo_l), hl & (a > hi_l), hu & (c < lo_u), hu & (c > hi_u)


def clip_active(s_new, zl, zu, dzl, dzu, az, mu, lo, hi, cfg=None):
    """Rows on which the clip of update() changes z_l or z_u."""
    a, b, c, d = clip_sides(s_new, zl, zu, dzl, dzu, az, mu, lo, hi, cfg)
    return a | b | c | d


def next_mu(mu, alpha, cfg):
    """Behind a step longer than 0.3: Ipopt's monotone rule max(max(mu_min, tol), min(0.2 mu, mu^1.5)) with mu_superlinear,
    max(mu_min, 0.2 mu) without; otherwise mu stays."""
    if not alpha > MU_STEP:
        return mu
    if cfg.mu_superlinear:
        return max(max(cfg.mu_min, cfg.tol), min(0.2 * mu, mu * np.sqrt(mu)))
    return max(cfg.mu_min, 0.2 * mu)


def new_decisions():
    """State of the decisions in front of the first step."""
    return dict(kind=0, banned=False, run=0, held=False, jam=0, best_viol=np.inf, best_it=0)


def next_kind(cfg, d, it, alpha, viol_before, viol_after, theta_after):
    """The decisions behind step number `it` (0-based) of kind d["kind"] (0 a fresh factorisation, 1 a chord step; a chord
    step that came out shorter than 1 is discarded: alpha 0, kind 2 in the history).  Returns the state in front of the next
    step, with "stop": None, "converged", "stalled" or "jammed" and "rejected".

      chord step next: chord_tol > 0, no chord step of this solve was discarded, this step was a full one (alpha = 1) to a
        violation <= chord_tol, and it was a fresh factorisation's -- or a chord step's with fewer than chord_max chord steps
        on this factorisation so far and a violation <= chord_shrink x the one in front of it
      hold: latched once an iterate number >= foothold_hold_from has a violation <= foothold_hold_tol
      jam: steps in a row shorter than stall_alpha (a discarded chord step breaks the row); two stop the solve
      stall: stall_iters iterations without a new lowest violation stop the solve"""
    was_chord = d["kind"] == 1
    rejected = was_chord and alpha != 1.0
    n = dict(d)
    n["rejected"] = rejected
    n["banned"] = d["banned"] or rejected
    n["run"] = d["run"] + 1 if was_chord else 0
    full = (not rejected) and alpha == 1.0
    chord = (cfg.chord_tol > 0 and not n["banned"] and full and viol_after <= cfg.chord_tol and
             (not was_chord or (n["run"] < cfg.chord_max and viol_after <= cfg.chord_shrink * viol_before)))
    n["kind"] = 1 if chord else 0
    n["held"] = bool(d["held"] or (cfg.foothold_hold_from > 0 and it + 1 >= cfg.foothold_hold_from and viol_after <= cfg.foothold_hold_tol))
    n["jam"] = d["jam"] + 1 if (cfg.stall_alpha > 0 and not rejected and alpha < cfg.stall_alpha) else 0
    conv = viol_after <= cfg.tol and theta_after <= cfg.tol
    improved = not conv and viol_after < d["best_viol"]
    if improved:
        n["best_viol"], n["best_it"] = viol_after, it + 1
    n["stop"] = ("converged" if conv else
                 "stalled" if (not improved and cfg.stall_iters > 0 and it + 1 - n["best_it"] >= cfg.stall_iters) else
                 "jammed" if n["jam"] >= 2 else None)
    return n


# ---- the whole iteration ---------------------------------------------------------------------------------------------
def solve(O, q, cfg, x0=None, max_iter=None, eps_rows=None):
    """The solve of problem q of oracle O with the settings of cfg, from towr's straight-line guess or from given nodes x0
    (then a warm start).  Returns a dict: states (one per iterate: x, g, s, zl, zu by inequality row, y by equality row -- of the
    KKT solve behind the step that led there --, mu, viol, theta, compl, held), events (one per step: kind, rejected, alpha, az, amax, trials, margins, clip rows, mu floor reached), status (0
    converged, 1 otherwise), iters, x (the result: the best iterate of a stalled or jammed solve) and the working set."""
    max_iter = cfg.max_iter if max_iter is None else max_iter
    free, E, I, lo, hi, kind = working_set(O, q)
    lo_i, hi_i = lo[I], hi[I]
    xl, xh = O.var_bounds(q)
    x = O.initial_guess(q) if x0 is None else np.array(x0, float)
    x[xl == xh] = xl[xl == xh]
    if O.swing_start_on_rule:
        x = O.project_swings(x)
    eps = np.full(len(E), cfg.eps_dual) if eps_rows is None else eps_rows
    hold_vars = np.isin(free, stance_foothold_vars(O, cfg))
    g = O.constraints(x)
    s_all, zl_all, zu_all, mu, viol, theta = start_state(g, lo, hi, kind, cfg, x0 is not None)
    s, zl, zu = s_all[I], zl_all[I], zu_all[I]
    d = new_decisions()
    d["best_viol"] = viol if not (viol <= cfg.tol and theta <= cfg.tol) else np.inf
    xbest = x.copy()
    states, events = [], []
    y = np.zeros(len(E))                          # the equality rows' multipliers of the last KKT solve (none yet: 0)

    def snap(held):
        states.append(dict(x=x.copy(), g=g.copy(), s=s.copy(), zl=zl.copy(), zu=zu.copy(), mu=mu, viol=viol, theta=theta,
                           compl=measures(g[I], s, zl, zu, lo_i, hi_i, g[E])[2], held=held, y=y.copy()))
    snap(False)
    status, it = 1, 0
    if viol <= cfg.tol and theta <= cfg.tol:
        status = 0
    K = lu = None
    stop = None
    while status and it < max_iter:
        J = O.jacobian(x)
        sig, w = np.zeros(O.m), np.zeros(O.m)
        sig[I], w[I] = barrier_terms(g[I], s, zl, zu, mu, lo_i, hi_i)
        chord = d["kind"] == 1
        rhs = kkt_rhs(J, g, free, E, I, w)
        if not chord:
            diag = np.where(hold_vars & d["held"], cfg.foothold_hold_weight, cfg.delta_x)
            K, lu = kkt_matrix(J, free, E, I, sig, diag, eps), None
        hp, _, lu = solve_refined(K, rhs, lu)
        dx = np.zeros(O.n)
        dx[free] = hp[:len(free)].astype(np.float64)
        y = hp[len(free):].astype(np.float64)     # (a discarded chord step's too: the solve was made)
        ds, dzl, dzu = slack_and_dual_steps(J[I], dx, g[I], s, zl, zu, mu, lo_i, hi_i)
        amax, az = step_lengths(s, ds, zl, zu, dzl, dzu, mu, lo_i, hi_i)
        alpha, trials, log = line_search(O.constraints, x, dx, s, ds, amax, (E, I))
        viol_before = viol
        if chord and alpha != 1.0:
            alpha_t, az_t = 0.0, 0.0
        else:
            alpha_t, az_t = alpha, az
            x = x + alpha * dx
            g = O.constraints(x)
        clip = np.nonzero(clip_active(s + alpha_t * ds, zl, zu, dzl, dzu, az_t, mu, lo_i, hi_i, cfg))[0]
        s, zl, zu = update(s, ds, zl, zu, dzl, dzu, alpha_t, az_t, mu, lo_i, hi_i, cfg)
        mu_new = next_mu(mu, alpha_t, cfg)
        floor = cfg.mu_superlinear and mu_new == max(cfg.mu_min, cfg.tol) and alpha_t > MU_STEP
        mu = mu_new
        viol, theta, _ = measures(g[I], s, zl, zu, lo_i, hi_i, g[E])
        d = next_kind(cfg, d, it, alpha_t, viol_before, viol, theta)
        events.append(dict(kind=2 if d["rejected"] else int(chord), rejected=d["rejected"], alpha=alpha_t, az=az_t, amax=amax,
                           trials=trials, log=log, clip_rows=clip, mu_floor=bool(floor), held=d["held"], next_kind=d["kind"]))
        it += 1
        snap(d["held"])
        if d["best_it"] == it:
            xbest = x.copy()
        stop = d["stop"]
        if stop == "converged":
            status = 0
        if stop:
            break
    out_x = xbest if stop in ("stalled", "jammed") else x
    return dict(states=states, events=events, status=status, iters=it, x=out_x, stop=stop,
                free=free, E=E, I=I, lo=lo, hi=hi, row_kind=kind)
