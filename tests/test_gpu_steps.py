"""Every interior-point step of k_start and k_step (csrc/kernels.hpp) against the restatement oracle/ipm.py, per formula and per
row, on the cases of step_cases.py.

Mechanism, no product change: planners with max_iter = 0 .. K make one plan call each on the same inputs.  A solve that runs
out of iterations exports its last iterate untouched (max_iter = 0: the starting state of k_start), so planner k hands out
state k -- nodes, and s, z_l, z_u through Planner.duals -- and the report's history gives mu, the step lengths, the trials, the
step kind and the measures.  The histories of the shorter planners equal the rows of the longest bit for bit (the prefixes are
prefixes).  The GPU's own step of an accepted iteration is recovered as dx = (x_{k+1} - x_k) / alpha, ds = (s_{k+1} - s_k) /
alpha, each off by at most one rounding of the updated value and one of the product alpha d, divided by alpha: the recovery
bound rb = u (|v_{k+1}| + |v_{k+1} - v_k|) / alpha, carried into every gate below (u = 2^-53).

Per step and problem, from the GPU's OWN state k (so that no error of an earlier step is forgiven or charged twice):
  1. start (k = 0): s against start_state on the oracle's constraint values at the exported nodes, gate GATE_VALUE + 4 u (1 +
     |lo| + |hi|) (the push is a clamp: 1-Lipschitz in g); mu against first_mu of the GPU's theta, 4 u; z against mu / gap of
     the GPU's own s and mu, 4 u; viol, theta GATE_VALUE; compl 4 u -- all relative where a quotient or product is compared
  2. direction: dx against the dense KKT solve (chord steps: the matrix of the factored iterate), 5e-6 of the step's largest
     entry (header of test_gpu_parity.py) + rb; reduced system: eps 1e-13 on the rows structure() no longer marks as equalities
  3. ds against J_I dx + (g - s): per row GATE_ENTRY x the 1-norm of dx over the row + GATE_VALUE + |J_I| rb_x + rb_s + the
     rounding of the row's sum (entries + 2) u (|J_I| |dx| + |g| + |s|)
  4. amax, az: the interval the ratio tests give when ds moves within rb_s and dz within (z / gap) rb_s + 4 u (|mu / gap| +
     |z| + |z / gap ds|), widened by 8 u; amax of the GPU = alpha_pr x 2^(trials - 1)
  5. line search: every trial the GPU made, evaluated through the oracle at the GPU's x_k + alpha dx: the accepted one meets
     the Armijo test, every earlier one fails it; decisions within rows x GATE_VALUE of the right-hand side would be excluded,
     and none may be (test_step_cpu.py holds the reference alone to that)
  6. update: z of state k + 1 against update(), per row az x the dz bound of 4. + 4 u (|z| + az |dz| + |z_new|); a row the clip
     of z acts on (the discard_* / clip_* cases: kappa_sigma 10 and 2) against its limit mu_k / (kappa gap) or kappa mu_k / gap
     at the GPU's own s_{k+1}, 4 u relative + the limit's sensitivity to rb_s, reported as `z_l clip` / `z_u clip`; mu against
     next_mu, 4 u; viol, theta of the history against measures on the oracle's g at x_{k+1}, GATE_VALUE; compl 4 u.  A
     discarded chord step leaves x, s, z and mu bit for bit (state k + 1 equals state k), and the step behind it is a fresh
     factorisation's, held to the dense solve at that same iterate
  7. decisions: the kind of every step, the stop, the factorisation / chord-solve totals against next_kind fed the history's
     own numbers (equalities); the hold latch enters 2. through the diagonal
  8. dual infeasibility: history row k (bit for bit the report's figure of prefix planner k) against oracle/duals.py at the
     GPU's own state k -- the oracle's Jacobian at the exported nodes, the basis Z of the system's unknowns (B-spline
     coefficients and footholds on the reduced system; step_cases.basis), y, z_l, z_u of Planner.duals.  Gate: the largest
     over the unknowns of GATE_ENTRY (bilinear cases: GATE_ENTRY_BILINEAR) x sum |Z| |v| + (terms + 4) u sum |Z| |J| |v|,
     derived like 3. (step_cases.dual_measure).  Row 0 is k_start's (no solve yet: y = 0, asserted).  A discarded chord step
     leaves x, s, z where they were, but its row does NOT repeat the preceding row's figure: k_step forms the measure behind
     every step with the multipliers of the solve it has just made, so row k + 1 carries the discarded chord solve's y at the
     iterate that stayed.  Held as every other row: Planner.duals of prefix planner k + 1 hands out that y.  The `hold` case
     runs with the hold weight in the stream's diagonal entries: a diagonal read as a Jacobian entry would show as 1e6
  9. y: exactly 0 on the rows structure() does not mark as equalities; on the others against the multipliers of the dense
     solve of 2. at state k - 1 (a discarded chord step: the chord solve's), GATE_DIRECTION of the dense y's largest entry --
     dx and y are one solve vector -- unless solve_refined and the unrefined LAPACK solve of the same matrices differ by more
     than GATE_DIRECTION / GATE_FACTOR of it somewhere in the case: then GATE_FACTOR x that spread (step_cases.y_gate_of).
     The multipliers are the report's only -- no plan depends on them, the dual infeasibility does.  On the bilinear map this
     check found the multiplier of a stance's terrain row off by 2.7 where the dense solve has 7e-5 and the largest multiplier
     is 2.3 (bilinear_1s problem 3, row 34: 2.4e5 times the gate; bilinear_steps 53 times, bilinear_no_qo 1.008 times), with dx
     and every other multiplier at the dense solve's values and the library's own k_residual at 0.60: the row was keyed at the
     stance's first node and so eliminated in front of its foothold with the pivot -eps_dual, y = -(g + J dx) / eps_dual, where
     an error of 7e-9 in the foothold's step (the terrain's slope of 2.75 in J) is 2.7.  model.hpp keys such a row behind its
     foothold on a bilinear map since (test_duals_cpu.py holds the order)
 10. ||d||: history column 3 of an accepted step against max |(x_{k+1} - x_k) / alpha| over the free variables, within rb; a
     discarded step (alpha = 0) leaves nothing to recover it from: counted and reported
Figures of 8. to 10.: profiles/dual_accuracy.json, with the groups of unknowns that attained the maximum per case.

What state k is: the export of a solve at its LAST iteration.  k_step takes its speculative first trial (spec: the trial
point evaluated with its Jacobian, lin_done, no gt -> g copy, the hold weight patched into the stream) only where another
iteration follows (it + 1 < max_iter), and a last iteration returns in front of the linearisation and the barrier-weight pass.
Every exported x, s, z therefore comes from a non-speculative step that ran the gt -> g copy; the speculative path runs at the
interior iterations of the longer planners and is seen through two things only: their history rows equal the shorter planners'
bit for bit, and the next step's dx -- computed by the KKT kernels from the stream and barrier weights the speculative step
left -- meets the dense solve at 5e-6.  The barrier weights sig, w themselves are not read back.

A failure names quantity, problem, step, constraint row and list position -- positions from KR x ET = 1024 on are tail rows
(through memory), the rest register rows.  Figures: profiles/step_accuracy.json (largest achieved / bound per case)."""
import dataclasses

import numpy as np
import pytest
from scipy.linalg import lu_solve

import step_cases as stc
from oracle import duals, ipm

pytestmark = pytest.mark.gpu
U = stc.U
TAIL = stc.KR * stc.ET
INF_DU = 9                                 # capi.HIST_NAMES: the history's dual-infeasibility column


def _gpu_states(c, cfg):
    """Per k = 0 .. K: (nodes, status, iters, s, zl, zu, [(report, history)], row kinds, free-variable flags)."""
    from qtos_amd.capi import Planner
    out = []
    for k in range(c.steps + 1):
        P = Planner(dataclasses.replace(cfg, max_iter=k), max_batch=c.B)
        try:
            if c.terrain is not None:
                P.set_heightfields(c.terrain[0], c.terrain[1])
            P.set_report(True)
            nodes, status, iters, _ = P.plan(c.start, c.goal, warm=c.warm)
            s, zl, zu, y = P.duals(c.B)             # (before any debug_* call: those reuse the workspace)
            reps = [P.report(b) for b in range(c.B)]
            rk, vf, _ = P.structure()
        finally:
            P.close()
        out.append(dict(x=nodes, status=status, iters=iters, s=s, zl=zl, zu=zu, y=y, reps=reps, rk=rk, vf=vf))
    return out


class Worst:
    def __init__(self):
        self.ratio, self.fails = {}, []

    def check(self, what, achieved, bound, where):
        """achieved <= bound, elementwise; keeps the largest achieved / bound and the first offender."""
        achieved, bound = np.atleast_1d(np.asarray(achieved, float)), np.atleast_1d(np.asarray(bound, float))
        bound = np.broadcast_to(bound, achieved.shape)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(achieved == 0, 0.0, achieved / bound)
        r = np.where(np.isnan(r), np.inf, r)
        i = int(np.argmax(r))
        self.ratio[what] = max(self.ratio.get(what, 0.0), float(r[i]))
        if not r[i] <= 1.0:
            self.fails.append((what, where(i) if callable(where) else where, float(achieved[i]), float(bound[i])))


def _interval(num, den, e_den, on, tau):
    """[lo, hi] of min(1, min over the rows `on` with den > 0 of tau num / den) when den moves within +- e_den."""
    with np.errstate(divide="ignore", invalid="ignore"):
        up, dn = den + e_den, den - e_den
        lo = np.where(on & (up > 0), tau * num / np.where(up > 0, up, 1.0), np.inf)
        hi = np.where(on & (dn > 0), tau * num / np.where(dn > 0, dn, 1.0), np.inf)
    return min(1.0, float(lo.min(initial=np.inf)) * (1 - 8 * U)), min(1.0, float(hi.min(initial=np.inf)) * (1 + 8 * U))


def _row(I):
    def where(b, k):
        return lambda i: dict(problem=b, step=k, row=int(I[i]), position=int(i), path="tail" if i >= TAIL else "registers")
    return where


def _check_case(name, reduced):
    c = stc.case(name)
    cfg = c.cfg if reduced else c.cfg_full
    G = _gpu_states(c, cfg)
    K, last = c.steps, G[c.steps]
    W = Worst()
    excluded = decisions = clipped_rows = clipped_tail = discarded = no_dnorm = 0
    Z, col_group = stc.basis(name, (True, True) if reduced else (False, False))
    attained, y_spread, y_checks = set(), 0.0, []
    for b in range(c.B):
        R = stc.run(name, b)                        # (the working set and the bounds; the GPU's own states are what is checked)
        free, E, I, lo, hi = R["free"], R["E"], R["I"], R["lo"][R["I"]], R["hi"][R["I"]]
        where = _row(I)
        hl, hu = ipm.has_bounds(lo, hi)
        rep, hist = last["reps"][b]
        steps = min(K, int(last["iters"][b]))
        assert len(hist) == steps + 1 and rep.iterations == steps
        # the prefixes are prefixes; the working set is the restatement's
        for k in range(K + 1):
            n = min(k, steps) + 1
            assert np.array_equal(G[k]["reps"][b][1][:n], hist[:n], equal_nan=True), (name, b, k)
            assert int(G[k]["iters"][b]) == n - 1
        assert np.array_equal(np.nonzero(last["vf"] != 0)[0], free)
        assert np.array_equal(np.nonzero(last["rk"] == 2)[0], I)
        if not reduced:
            assert np.array_equal(np.nonzero(last["rk"] == 1)[0], E)
        assert (last["rk"][E] != 1).any() == reduced
        eps = np.where(last["rk"][E] == 1, cfg.eps_dual, 1e-13)
        hold_vars = np.isin(free, ipm.stance_foothold_vars(c.O, cfg))
        off_rows = np.setdiff1d(np.arange(c.O.m), I)

        def state(k):
            g = G[min(k, steps)]
            assert not g["s"][b][off_rows].any() and not g["zl"][b][off_rows].any() and not g["zu"][b][off_rows].any()
            return g["x"][b], g["s"][b][I], g["zl"][b][I], g["zu"][b][I]

        def dual_state(k):
            # 8. the dual infeasibility of history row k against the restatement at the GPU's own state k; 9. y off the equality rows
            g = G[min(k, steps)]
            assert g["reps"][b][0].dual_infeasibility == hist[min(k, steps)][INF_DU], (name, b, k)
            assert not g["y"][b][last["rk"] != 1].any(), (name, b, k, "y off the rows structure() marks as equalities")
            val, col, gate = stc.dual_measure(c, Z, g["x"][b], g["y"][b], g["zl"][b], g["zu"][b])
            grp = duals.GROUPS[col_group[col]]
            attained.add(grp)
            W.check("inf_du", abs(hist[min(k, steps)][INF_DU] - val), gate, dict(problem=b, step=k, group=grp, restatement=val))
        # 1. the starting state
        x0, s0, zl0, zu0 = state(0)
        g0 = c.O.constraints(x0)
        s_ref = ipm.start_state(g0, R["lo"], R["hi"], R["row_kind"], cfg, c.warm is not None)[0][I]
        W.check("start_s", np.abs(s0 - s_ref), stc.GATE_VALUE + 4 * U * (1 + np.where(hl, np.abs(lo), 0) + np.where(hu, np.abs(hi), 0)), where(b, 0))
        viol, theta, compl = ipm.measures(g0[I], s0, zl0, zu0, lo, hi, g0[E])
        W.check("start_viol", abs(hist[0][0] - viol), stc.GATE_VALUE, (b, 0))
        W.check("start_theta", abs(hist[0][1] - theta), stc.GATE_VALUE, (b, 0))
        mu0 = hist[0][2]
        W.check("start_mu", abs(mu0 - ipm.first_mu(hist[0][1], cfg)), 4 * U * mu0, (b, 0))
        _, _, dl, du = ipm.gaps(s0, lo, hi)
        W.check("start_zl", np.abs(zl0 - np.where(hl, mu0 / dl, 0.0)), 4 * U * np.abs(zl0), where(b, 0))
        W.check("start_zu", np.abs(zu0 - np.where(hu, mu0 / du, 0.0)), 4 * U * np.abs(zu0), where(b, 0))
        W.check("start_compl", abs(hist[0][8] - compl), 4 * U * compl, (b, 0))
        assert not G[0]["y"][b].any()                       # (k_start's row 0: no KKT solve yet)
        dual_state(0)
        d = ipm.new_decisions()
        d["best_viol"] = hist[0][0]
        Kmat = lu = None
        kinds = []
        for k in range(steps):
            h, mu = hist[k + 1], hist[k][2]
            alpha, az, trials, kind = h[4], h[5], int(h[6]), int(h[7])
            x1, s1, zl1, zu1 = state(k + 1)
            g1 = c.O.constraints(x1)
            # 7. the kind of this step
            assert kind == (2 if d["kind"] == 1 and alpha != 1.0 else d["kind"]), (name, b, k, kind, d)
            kinds.append(kind)
            J = c.O.jacobian(x0)
            sig, w = np.zeros(c.O.m), np.zeros(c.O.m)
            sig[I], w[I] = ipm.barrier_terms(g0[I], s0, zl0, zu0, mu, lo, hi)
            rhs_k = ipm.kkt_rhs(J, g0, free, E, I, w)
            if kind == 0:
                Kmat = ipm.kkt_matrix(J, free, E, I, sig, np.where(hold_vars & d["held"], cfg.foothold_hold_weight, cfg.delta_x), eps)
                lu = None
            if kind == 2:
                # 6. a discarded chord step leaves the iterate bit for bit: state k + 1 IS state k, mu included (al = az = 0
                # in update_row: s + 0 ds, z + 0 dz, and the clip at the old gap and mu finds z where the last step left it).
                # The step behind it is then checked like any other: a fresh factorisation (7.) whose direction meets the
                # dense solve AT THIS ITERATE (2.: the linearisation ran at x, not at the trial point), no chord step after
                assert alpha == 0.0 and az == 0.0 and h[2] == mu, (name, b, k, alpha, az, h[2], mu)
                assert np.array_equal(x1, x0) and np.array_equal(s1, s0) and np.array_equal(zl1, zl0) and np.array_equal(zu1, zu0), (name, b, k)
                assert h[0] == hist[k][0] and h[1] == hist[k][1], (name, b, k, "viol / theta of an iterate that did not move")
                discarded += k + 1 < steps
                # 10. the direction of a discarded step is not applied: nothing to recover its largest entry from
                no_dnorm += 1
                hp, _, lu = ipm.solve_refined(Kmat, rhs_k, lu)          # (9.: the chord solve was made, and its y is in the next row)
            else:
                xd = x1.astype(np.longdouble) - x0
                sd = s1.astype(np.longdouble) - s0
                dx, ds = (xd / alpha).astype(np.float64), (sd / alpha).astype(np.float64)
                rb_x = U * (np.abs(x1) + np.abs(xd).astype(np.float64)) / alpha + U * np.abs(dx)
                rb_s = U * (np.abs(s1) + np.abs(sd).astype(np.float64)) / alpha + U * np.abs(ds)
                # 2. the direction
                hp, _, lu = ipm.solve_refined(Kmat, rhs_k, lu)
                ref = hp[:len(free)].astype(np.float64)
                scale = np.abs(ref).max()
                assert not dx[np.setdiff1d(np.arange(c.O.n), free)].any()
                W.check("dx_chord" if kind == 1 else "dx", np.abs(dx[free] - ref), stc.GATE_DIRECTION * scale + rb_x[free],
                        lambda i, b=b, k=k: dict(problem=b, step=k, variable=int(free[i])))
                # 10. the history's ||d||: the largest entry of the direction
                W.check("dnorm", abs(h[3] - np.abs(dx[free]).max()), rb_x[free].max(), (b, k))
                # 3. ds
                JI = J[I]
                aJ, adx = np.abs(JI), np.abs(dx)
                ds_ref = (JI.astype(np.longdouble) @ dx.astype(np.longdouble)).astype(np.float64) + (g0[I] - s0)
                bound = (stc.GATE_ENTRY * ((JI != 0) @ adx) + stc.GATE_VALUE + aJ @ rb_x + rb_s +
                         ((JI != 0).sum(axis=1) + 2) * U * (aJ @ adx + np.abs(g0[I]) + np.abs(s0)))
                W.check("ds", np.abs(ds - ds_ref), bound, where(b, k))
                # 4. the two ratio tests, on the GPU's own s, ds, z, mu
                tau = max(0.99, 1.0 - mu)
                _, _, dl, du = ipm.gaps(s0, lo, hi)
                dzl, dzu = ipm.dual_steps(s0, ds, zl0, zu0, mu, lo, hi)
                e_dzl = np.where(hl, zl0 / dl * rb_s + 4 * U * (np.abs(mu / dl) + np.abs(zl0) + np.abs(zl0 / dl * ds)), 0.0)
                e_dzu = np.where(hu, zu0 / du * rb_s + 4 * U * (np.abs(mu / du) + np.abs(zu0) + np.abs(zu0 / du * ds)), 0.0)
                amax_ref, az_ref = ipm.step_lengths(s0, ds, zl0, zu0, dzl, dzu, mu, lo, hi)
                a_lo = min(_interval(dl, -ds, rb_s, hl, tau)[0], _interval(du, ds, rb_s, hu, tau)[0])
                a_hi = min(_interval(dl, -ds, rb_s, hl, tau)[1], _interval(du, ds, rb_s, hu, tau)[1])
                z_lo = min(_interval(zl0, -dzl, e_dzl, hl, tau)[0], _interval(zu0, -dzu, e_dzu, hu, tau)[0])
                z_hi = min(_interval(zl0, -dzl, e_dzl, hl, tau)[1], _interval(zu0, -dzu, e_dzu, hu, tau)[1])
                amax = alpha * 2.0 ** (trials - 1)
                assert a_lo <= amax_ref <= a_hi and z_lo <= az_ref <= z_hi
                W.check("amax", abs(amax - amax_ref), max(a_hi - amax_ref, amax_ref - a_lo) if a_lo <= amax <= a_hi else 0.0, (b, k, amax, amax_ref))
                W.check("az", abs(az - az_ref), max(z_hi - az_ref, az_ref - z_lo) if z_lo <= az <= z_hi else 0.0, (b, k, az, az_ref))
                # 5. the line search
                margin = stc.exclusion_margin(len(E) + len(I))
                th0 = ipm.l1_infeasibility(g0, s0, E, I)
                for t in range(trials):
                    al = amax * 0.5 ** t
                    th = ipm.l1_infeasibility(c.O.constraints(x0 + al * dx), s0 + al * ds, E, I)
                    rhs = (1.0 - ipm.ARMIJO * al) * th0
                    decisions += 1
                    ok = stc.armijo_decision(th, rhs, margin)
                    if ok is None:
                        excluded += 1
                        continue
                    if t < trials - 1:
                        assert not ok, ("an earlier trial meets the Armijo test", name, b, k, t, th, rhs)
                    elif trials < ipm.MAX_TRIALS:
                        assert ok, ("the accepted trial fails the Armijo test", name, b, k, t, th, rhs)
                # 6. the update of z and mu.  The clip's limits are formed from the GPU's OWN new slack and the OLD mu (update_row
                # clips at sn, which it stores, before mu moves): a row the clip acts on -- z + az dz of the GPU's own state k
                # outside the band -- is held to its limit at 4 u relative (the gap, one product, one quotient) plus the limit's
                # sensitivity |limit| / gap to the slack step's recovery bound; a row whose z + az dz is within the dz bound of a
                # limit may fall either side of it and takes the larger of the two bounds; every other row the dz bound alone
                lim = ipm.clip_limits(s1, mu, lo, hi, cfg)
                _, _, dl1, du1 = ipm.gaps(s1, lo, hi)
                for zn, has, z0, dz, e_dz, z1, gap1, lim_lo, lim_hi in (("l", hl, zl0, dzl, e_dzl, zl1, dl1, lim[0], lim[1]),
                                                                      ("u", hu, zu0, dzu, e_dzu, zu1, du1, lim[2], lim[3])):
                    un = z0 + az * dz
                    ref = np.where(has, np.minimum(np.maximum(un, lim_lo), lim_hi), un)
                    b_dz = az * e_dz + 4 * U * (np.abs(z0) + az * np.abs(dz) + np.abs(ref))
                    b_clip = 4 * U * np.abs(ref) + np.abs(ref) / gap1 * alpha * rb_s
                    clipped = has & ((un < lim_lo) | (un > lim_hi))
                    near = has & ((np.abs(un - lim_lo) <= b_dz) | (np.abs(un - lim_hi) <= b_dz))
                    bound = np.where(near, np.maximum(b_dz, b_clip), np.where(clipped, b_clip, b_dz))
                    err = np.abs(z1 - ref)
                    rows_c, rows_f = np.nonzero(clipped)[0], np.nonzero(~clipped)[0]
                    W.check("z" + zn, err[rows_f], bound[rows_f], lambda i, f=where(b, k), r=rows_f: f(r[i]))
                    # (register rows and tail rows apart: a failure names its worst row on either path)
                    for r in (rows_c[rows_c < TAIL], rows_c[rows_c >= TAIL]):
                        if len(r):
                            W.check("z_%s clip" % zn, err[r], bound[r], lambda i, f=where(b, k), r=r: f(r[i]))
                    if alpha > ipm.MU_STEP:                    # (mu moves behind this step: the limits at the new mu are others)
                        clipped_rows += len(rows_c)
                        clipped_tail += int((rows_c >= TAIL).sum())
                W.check("mu", abs(h[2] - ipm.next_mu(mu, alpha, cfg)), 4 * U * h[2], (b, k))
            viol, theta, compl = ipm.measures(g1[I], s1, zl1, zu1, lo, hi, g1[E])
            W.check("viol", abs(h[0] - viol), stc.GATE_VALUE, (b, k))
            W.check("theta", abs(h[1] - theta), stc.GATE_VALUE, (b, k))
            W.check("compl", abs(h[8] - compl), 4 * U * compl, (b, k))
            # 9. y of this step's solve (state k + 1 hands it out) against the dense solve's, on the rows the system keeps as
            # equalities; the two dense solves' own spread decides the gate once the case is through
            on = last["rk"][E] == 1
            y_ref = hp[len(free):].astype(np.float64)[on]
            y_spread = max(y_spread, float(np.abs(lu_solve(lu, rhs_k)[len(free):][on] - y_ref).max() / np.abs(y_ref).max()))
            y_checks.append((np.abs(G[k + 1]["y"][b][E[on]] - y_ref), np.abs(y_ref).max(), b, k, E[on]))
            dual_state(k + 1)
            # 7. the decisions behind this step, from the history's own numbers
            d = ipm.next_kind(cfg, d, k, alpha, hist[k][0], h[0], h[1])
            assert d["stop"] in (None, "converged")           # (the stall rules are off)
            if d["stop"]:
                assert k + 1 == steps and rep.status == 0 and last["status"][b] == 0, (name, b, k)
            else:
                assert k + 1 < steps or steps == K, (name, b, k, "the solve stopped where the restatement goes on")
            x0, s0, zl0, zu0, g0 = x1, s1, zl1, zu1, g1
        if steps < K or d.get("stop"):
            assert d["stop"] == "converged" and rep.status == 0
        else:
            assert rep.status == 1
        assert rep.n_factorizations == kinds.count(0) and rep.n_chord_solves == len(kinds) - kinds.count(0)
    y_gate = stc.y_gate_of(y_spread)
    for err, scale, b, k, rows in y_checks:
        W.check("y", err, y_gate * scale, lambda i, b=b, k=k, rows=rows: dict(problem=b, step=k, row=int(rows[i])))
    stc.record_dual("gpu_reduced" if reduced else "gpu_full", name,
                    dict(achieved_over_bound={q: W.ratio.get(q, 0.0) for q in ("inf_du", "y", "dnorm")}, y_cpu_spread=y_spread, y_gate=y_gate,
                         attaining_groups=sorted(attained), rows_of_discarded_steps_without_dnorm=no_dnorm, problems=c.B, steps=K))
    stc.record("gpu_reduced" if reduced else "gpu_full", name,
               dict(problems=c.B, steps=K, armijo_decisions=decisions, excluded=excluded, achieved_over_bound=W.ratio,
                    clipped_rows_checked_while_mu_moves=clipped_rows, of_them_tail_rows=clipped_tail,
                    discarded_chord_steps_with_a_step_behind=discarded, dual_infeasibility_attained_by=sorted(attained)))
    assert excluded == 0
    # the case is on the GPU where the restatement's run put it on the CPU (test_the_case_table_sits_on_the_paths_it_names)
    if name in stc.CLIP_NAMES:
        assert clipped_rows > 0 and (c.n_iq <= TAIL or 0 < clipped_tail < clipped_rows), (name, clipped_rows, clipped_tail)
    else:
        assert clipped_rows == 0, (name, "the clip acts where kappa_sigma is Ipopt's 1e10")
    assert (discarded > 0) == (name in stc.DISCARD_NAMES), (name, discarded)
    assert not W.fails, W.fails[:12]


@pytest.mark.parametrize("name", stc.DUAL_NAMES)
def test_every_step_of_the_full_system_matches_the_restatement(name):
    _check_case(name, False)


@pytest.mark.parametrize("name", stc.DUAL_REDUCED_NAMES)
def test_every_step_of_the_reduced_system_matches_the_restatement(name):
    _check_case(name, True)


def _groups():
    """STOPPED by (case, settings): the problems of a case run as one batch."""
    out = {}
    for e in stc.STOPPED:
        out.setdefault((e[0], tuple(sorted(e[2].items()))), []).append(e)
    return list(out.values())


@pytest.mark.parametrize("entries", _groups(), ids=lambda es: "%s-%s" % (es[0][0], "-".join(sorted({str(e[3]) for e in es}))))
def test_a_stopped_solve_stops_where_the_restatement_stops_and_hands_back_its_best_iterate(entries):
    """The cases run with the stall rules off.  Here the problems of a step_cases.STOPPED case run with the entry's settings --
    bilinear_steps with the product's (stall_iters = 5, stall_alpha = 1e-2, max_iter = 24: problem 1 stalls in its ninth
    iteration), the jam entries with stall_alpha = 0.9 or, far_goal, the product's own 1e-2 -- next to a run without the stall
    rules.  In front of a stop every history row is that of the rules-off run bit for bit, and so is the stop row in every
    column the step writes (its dual infeasibility is k_report's, of the nodes handed back); the stop is where next_kind, fed
    the history's own numbers, puts it, and for the entries' problems where the restatement's own run puts it, of the kind and
    in the iteration the table names; the nodes handed back are those of the iterate with the lowest violation, bit for bit
    what a planner out of iterations at that iterate exports, with that violation (a jammed solve may have improved in its
    last step: then that one); status 1; the last two steps of a jammed solve are shorter than stall_alpha.  The entries
    that must NOT stop (discard_bilinear under stall_alpha = 0.9: alpha 1, 0 -- the discarded chord step --, 0.25, 1 ...) run
    to the rules-off result bit for bit: the discarded step does not count."""
    from qtos_amd.capi import Planner
    name = entries[0][0]
    c = stc.case(name)
    cfg_on = stc.stopped_cfg(entries[0])
    cfg_off = stc.prefix(cfg_on)
    assert cfg_on.stall_alpha > 0 and cfg_off.max_iter == cfg_on.max_iter and cfg_off.stall_alpha == 0 and cfg_off.stall_iters == 0
    if entries[0][3] == "stalled":
        assert cfg_on.stall_iters > 0 and cfg_on == c.product_full      # (the product's settings)

    def plan(cfg):
        P = Planner(cfg, max_batch=c.B)
        try:
            if c.terrain is not None:
                P.set_heightfields(c.terrain[0], c.terrain[1])
            P.set_report(True)
            nodes, status, iters, viol = P.plan(c.start, c.goal)
            return dict(x=nodes, status=status, iters=iters, viol=viol, reps=[P.report(b) for b in range(c.B)])
        finally:
            P.close()
    on, off = plan(cfg_on), plan(cfg_off)
    stops, best_its = {}, {}
    for b in range(c.B):
        rep, hist = on["reps"][b]
        n = len(hist)
        assert 1 <= n <= len(off["reps"][b][1]) and n - 1 == int(on["iters"][b]) == rep.iterations
        ref = off["reps"][b][1][:n]
        step_cols = [col for col in range(hist.shape[1]) if col != INF_DU]
        assert np.array_equal(hist[:n - 1], ref[:n - 1], equal_nan=True), b
        assert np.array_equal(hist[n - 1, step_cols], ref[n - 1, step_cols]), b         # everything the step itself writes
        d = ipm.new_decisions()
        d["best_viol"] = hist[0][0]
        for k in range(n - 1):
            h = hist[k + 1]
            assert int(h[7]) == (2 if d["kind"] == 1 and h[4] != 1.0 else d["kind"]), (b, k)
            d = ipm.next_kind(cfg_on, d, k, h[4], hist[k][0], h[0], h[1])
            if k + 1 < n - 1:
                assert d["stop"] is None, (b, k, d["stop"])
            elif n - 1 < cfg_on.max_iter:
                assert d["stop"] is not None, (b, k, "the solve stopped where the restatement goes on")
        stops[b] = d.get("stop")
        assert int(on["status"][b]) == rep.status == (0 if stops[b] == "converged" else 1)
        # the dual infeasibility of the stop row is the report's: k_report forms it for a finished solve, at the nodes it hands
        # back -- the last iterate, and then the stall-off run's own figure of that iterate, unless the solve stalled or
        # jammed: then the best iterate, and the report's final measure
        if stops[b] in ("stalled", "jammed"):
            assert hist[n - 1, INF_DU] == rep.dual_infeasibility, b
        else:
            assert np.array_equal(hist[n - 1, INF_DU], ref[n - 1, INF_DU], equal_nan=True), b
        if stops[b] in ("stalled", "jammed"):
            # the best iterate: what a planner out of iterations there exports
            best = best_its[b] = d["best_it"]
            assert hist[best][0] == d["best_viol"] == min(hist[:, 0]) and on["viol"][b] == d["best_viol"]
            assert n - 1 < len(off["reps"][b][1]) - 1                       # without the rule the solve goes on
            at_best = plan(dataclasses.replace(cfg_off, max_iter=best))
            assert np.array_equal(at_best["reps"][b][1], hist[:best + 1], equal_nan=True)
            assert np.array_equal(on["x"][b], at_best["x"][b]), b
        else:
            # no stop by a rule: the run IS the rules-off run
            assert n == len(off["reps"][b][1]) and np.array_equal(on["x"][b], off["x"][b]) and on["viol"][b] == off["viol"][b], b
            assert int(on["status"][b]) == int(off["status"][b])
        if stops[b] == "jammed":
            assert n >= 3 and hist[n - 1][4] < cfg_on.stall_alpha and hist[n - 2][4] < cfg_on.stall_alpha, (b, hist[:, 4])
            assert int(hist[n - 1][7]) != 2 and int(hist[n - 2][7]) != 2
    for _, b, _, stop, at in entries:
        assert stops[b] == stop and (at is None or int(on["iters"][b]) == at), (name, b, stops, on["iters"])
        R = stc.run(name, b, cfg_on)
        assert (R["stop"], R["iters"]) == (stop, int(on["iters"][b]))
        if stop == "converged":
            # the discarded chord step stood between a long step and a short one, and did not count
            al, kinds = on["reps"][b][1][1:, 4], on["reps"][b][1][1:, 7].astype(int)
            k = list(kinds).index(2)
            assert al[k] == 0.0 and 0 < al[k + 1] < cfg_on.stall_alpha <= al[k - 1] and int(on["status"][b]) == 0
    stc.record("gpu_stopped_solve", "%s %s" % (name, " ".join("%s=%s" % kv for kv in sorted(entries[0][2].items())) or "product settings"),
               dict(stops={str(b): v for b, v in stops.items()}, iterations=[int(i) for i in on["iters"]], best_iterates={str(b): int(v) for b, v in best_its.items()},
                    iterations_without_the_stall_rules=[int(i) for i in off["iters"]],
                    last_alphas={str(b): [float(a) for a in on["reps"][b][1][-2:, 4]] for b in range(c.B)}))
