"""The rollout rule in numpy (qtos_amd/rollout.py, what k_rollout is held to) on the CPU: closed forms of the semi-implicit sums,
the C oracle's force columns, an independent RK4 integrator for the order of the method, the carried state, the freeze.

The plans come as tests/test_plan_check_cpu.py gets them (tests/rollout_cases.py); the CSV rows the closed forms are made of come
from the C oracle's qo_sample, which is independent of the package's evaluator.  The gate is rollout_cases.gate: the larger of 8 x
the float64-vs-longdouble floor of the statement measured in the same test and the bound the test's docstring derives, capped
at 1e-10.  Measured floors: profiles/rollout_accuracy.json."""
import numpy as np
import pytest

import rollout_cases as rc
from rollout_cases import F64, LD, U

TILE = 256


def same(a, b):
    """Equal to the bit (a longdouble's padding bytes are not part of it; NaNs in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == F64:
        return a.shape == b.shape and a.tobytes() == np.asarray(b, F64).tobytes()
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def both(plan, hz, first, n, params, **kw):
    from qtos_amd import rollout as ro
    return {dt: ro.rollout_rows(plan.L, plan.x, 0.25, hz, first, n, params, dtype=dt, **kw) for dt in (F64, LD)}


def test_free_fall_is_the_closed_form_of_the_semi_implicit_sums():
    """ff_scale 0, no gains, 400 ticks at 200 Hz from row 100 of the golden walk with w_b = (0.3, -0.2, 0.5) rad/s.

    v_k = v_0 - g k h e_z and r_k = r_0 + k h v_0 - g h^2 k (k + 1) / 2 e_z exactly; the float64 rule forms them by k additions.
    Bound: |v| <= |v_0| + 2 g < 20 m/s, so an addition into v rounds by at most 20 u and the product h a by less: 400 x 21 u =
    8400 u on v; |r| < 20 m with a term h v that carries v's error times h = 5e-3: 400 x (20 u + 5e-3 x 8400 u + 1 u) < 25 600 u
    = 2.9e-12 m.  The world angular momentum R Ib_s w_b of a free body is constant; the explicit step keeps it to first order in
    h: its drift halves with h (ratios of successive substeps in 1.5 .. 2.5) and the float64 and longdouble drifts L_k - L_0 agree within
    the propagated bound (400 steps x 64 u of the largest entry, 0.5 x 0.025 kg m^2/s, at both ends of the difference)."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan("walk")
    hz, n, k0 = 200.0, 401, 100
    row0 = plan.O.sample(plan.x, 0.25, hz, k0 + 1)[k0]
    entry, drift = {}, {}
    for sub in (1, 2, 4):
        p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, ff_scale=0.0, substeps=sub)
        out = {}
        for dt in (F64, LD):
            s = ro.initial_state(row0, dt)
            s[10:13] = [dt(0.3), dt(-0.2), dt(0.5)]
            out[dt] = ro.rollout_rows(plan.L, plan.x, 0.25, hz, k0, n, p, state=s, dtype=dt)
            assert (out[dt][2] == 0).all()
        Ib = np.asarray(INERTIA_PHYSICAL, F64).astype(LD)
        Lw = {}
        for dt in (F64, LD):
            rows = out[dt][1].astype(LD)
            wb = np.stack([np.array(ro.quat_matrix(rows[j, 13:17])).reshape(3, 3).T @ rows[j, 10:13] for j in range(n)])   # R^T (R w_b)
            Lw[dt] = np.stack([np.array(ro.quat_matrix(rows[j, 13:17])).reshape(3, 3) @ (Ib @ wb[j]) for j in range(n)])
        drift[sub] = float(np.abs(Lw[LD] - Lw[LD][0]).max())
        if sub == 1:
            h, g = LD(1) / LD(hz), LD(F64(plan.cfg.gravity))
            k = np.arange(n).astype(LD)
            r0, v0 = row0[1:4].astype(LD), row0[19:22].astype(LD)
            v_want = v0[None] + np.outer(k, [0, 0, -g * h])
            r_want = r0[None] + np.outer(k * h, v0) + np.outer(k * (k + 1) / 2, [0, 0, -g * h * h])
            for name, cols, want, bound in (("v", slice(7, 10), v_want, 8400 * U), ("r", slice(1, 4), r_want, 25600 * U)):
                floor = rc.dist(out[F64][1][:, cols], out[LD][1][:, cols])
                err = rc.dist(out[F64][1][:, cols], want)
                entry[name] = dict(floor=floor, err=err, gate=rc.gate(floor, bound))
                assert err <= rc.gate(floor, bound), (name, err, floor)
                assert rc.dist(out[LD][1][:, cols], want) <= rc.gate(floor, bound)
            # the float64 drift against the longdouble drift, at the propagated bound alone (their distance is the floor itself:
            # a gate made of it would hold by construction)
            apart = rc.dist(Lw[F64] - Lw[F64][0], Lw[LD] - Lw[LD][0])
            bound = 2 * 400 * 64 * U * 0.0125
            entry["L_world"] = dict(apart=apart, bound=bound, drift=drift[1], drift_float64=float(np.abs(Lw[F64] - Lw[F64][0]).max()))
            assert apart <= bound < rc.CAP, (apart, bound)
    entry["L_drift_by_substeps"] = drift
    rc.record("cpu_free_fall", entry)
    assert 1.5 <= drift[1] / drift[2] <= 2.5 and 1.5 <= drift[2] / drift[4] <= 2.5, drift
    assert drift[1] < 0.05 * 0.0125                                                    # and small: 2 s of tumbling at 0.6 rad/s


@pytest.mark.parametrize("name", ["walk", "trot"])
@pytest.mark.parametrize("mass_scale", [1.0, 2.0])
def test_open_loop_translation_is_a_prefix_sum_of_the_oracles_forces(name, mass_scale):
    """No gains, 1000 rows at 1 kHz: v_K - v_0 = h sum_k (sum_e f_e,k / m_s - g e_z) over the oracle's force columns, by np.cumsum
    in longdouble.  Bound: |v| < 6 m/s (twice the mass: the body falls for a second), so each of the 1000 additions rounds by at most 6 u, and the product h a (|a| < 20) by
    0.02 u; the rule's forces come from the package's evaluator and the oracle's from its own: both are float64 evaluations of one
    cubic with |f| < 64 N, 32 u x 64 apart at the most, which enters v as h / m_s of it, 0.7 u: 1000 x 6.8 u = 6800 u."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan(name)
    hz, n = 1000.0, 1001
    p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL)
    out = both(plan, hz, 0, n, p, mass_scale=mass_scale)
    assert out[F64][5] == 0 and out[LD][5] == 0
    c = plan.O.sample(plan.x, 0.25, hz, n).astype(LD)
    assert np.abs(c[:, 25:37]).max() < 64
    m_s = LD(F64(plan.cfg.mass)) * LD(mass_scale)
    a = (c[:, 25:28] + c[:, 28:31] + c[:, 31:34] + c[:, 34:37]) / m_s
    a[:, 2] -= LD(F64(plan.cfg.gravity))
    want = np.concatenate([np.zeros((1, 3), LD), np.cumsum(a[:-1], axis=0, dtype=LD)]) / LD(hz)
    got = {dt: out[dt][1][:, 7:10].astype(LD) - out[dt][1][0, 7:10].astype(LD) for dt in (F64, LD)}
    floor, err = rc.dist(got[F64], got[LD]), rc.dist(got[F64], want)
    g = rc.gate(floor, 6800 * U)
    rc.record("cpu_prefix_sum_%s_x%g" % (name, mass_scale), dict(floor=floor, err=err, gate=g, err_longdouble=rc.dist(got[LD], want)))
    assert float(np.abs(out[LD][1][:, 7:10]).max()) < 6 and float(np.abs(a).max()) < 20
    assert err <= g and rc.dist(got[LD], want) <= g, (err, floor)
    assert np.array_equal(out[F64][1][:, 0], plan.O.sample(plan.x, 0.25, hz, n)[:, 0])      # the time stamps, to the bit


def test_push_changes_the_velocity_by_its_impulse():
    """(3, 0, 0) N over the ticks 100 .. 149 of an open loop at 1 kHz: v_x differs from the unpushed run by 3 x 50 h / m_s behind
    them, and bit 4 is set on exactly those rows.  Bound: two runs of 300 additions into |v| < 2: 2 x 300 x 2 u = 1200 u."""
    from qtos_amd import rollout as ro
    plan = rc.plan("walk")
    hz, n = 1000.0, 300
    p = ro.RolloutParams(plan.cfg, push_from=103, push_ticks=50)
    free = both(plan, hz, 0, n, p, count=3)
    hit = both(plan, hz, 0, n, p, count=3, push=(3.0, 0, 0, 0, 0, 0))
    want = LD(3) * 50 / LD(hz) / LD(F64(plan.cfg.mass))
    d = {dt: hit[dt][1][:, 7].astype(LD) - free[dt][1][:, 7].astype(LD) for dt in (F64, LD)}
    floor = rc.dist(d[F64], d[LD])
    g = rc.gate(floor, 1200 * U)
    rc.record("cpu_push", dict(floor=floor, err=float(abs(d[F64][-1] - want)), gate=g))
    assert abs(d[F64][-1] - want) <= g and abs(d[LD][-1] - want) <= g and (d[F64][:101] == 0).all()
    for dt in (F64, LD):
        assert np.array_equal(np.nonzero(hit[dt][2] & ro.PUSH)[0], np.arange(100, 150))
        assert not (free[dt][2] & ro.PUSH).any() and hit[dt][4] == 3 + n


# ---- an integrator of its own: longdouble RK4 on the continuous equations, quaternions as (w, x, y, z) ------------------------
def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1:] @ b[1:], *(a[0] * b[1:] + b[0] * a[1:] + np.cross(a[1:], b[1:]))], LD)


def _rot(q):
    w, v = q[0], q[1:]
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], LD)
    return np.eye(3, dtype=LD) + 2 * w * K + 2 * (K @ K)


def _inv3(a):
    c = np.array([[a[(i + 1) % 3, (j + 1) % 3] * a[(i + 2) % 3, (j + 2) % 3] - a[(i + 1) % 3, (j + 2) % 3] * a[(i + 2) % 3, (j + 1) % 3]
                   for i in range(3)] for j in range(3)], LD)
    return c / (a[0] @ c[:, 0])


def _plan_row(c):
    """(r_p, v_p, q_p (w, x, y, z), w_p, F, tau_p) of an oracle CSV row, by rotation matrices."""
    c = c.astype(LD)
    a, b, y = c[4], c[5], c[6]
    Rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]], LD)
    Ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]], LD)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], LD)
    q = _qmul(_qmul(np.array([np.cos(y / 2), 0, 0, np.sin(y / 2)], LD), np.array([np.cos(b / 2), 0, np.sin(b / 2), 0], LD)),
              np.array([np.cos(a / 2), np.sin(a / 2), 0, 0], LD))
    assert np.abs(_rot(q) - Rz @ Ry @ Rx).max() < 1e-17
    w = c[24] * np.array([0, 0, 1], LD) + Rz @ (c[23] * np.array([0, 1, 0], LD)) + Rz @ Ry @ (c[22] * np.array([1, 0, 0], LD))
    F, tau = np.zeros(3, LD), np.zeros(3, LD)
    for e in range(4):
        F += c[25 + 3 * e:28 + 3 * e]
        tau += np.cross(c[7 + 3 * e:10 + 3 * e] - c[1:4], c[25 + 3 * e:28 + 3 * e])
    return c[1:4], c[19:22], q, w, F, tau


def rk4_rollout(rows37, hz, mass, g, Ib, gains, per_tick=16):
    kpl, kdl, kpa, kda = (LD(gains[k]) for k in ("kp_lin", "kd_lin", "kp_ang", "kd_ang"))
    Ib = np.asarray(Ib, F64).astype(LD)
    Ii = _inv3(Ib)
    rp, vp, qp, wp, F, tp = _plan_row(rows37[0])
    y = np.concatenate([rp, vp, qp, _rot(qp).T @ wp])
    h = LD(1) / LD(hz) / per_tick

    def f(y):
        r, v, q, wb = y[0:3], y[3:6], y[6:10], y[10:13]
        R = _rot(q / np.sqrt(q @ q))
        e = r - rp
        acc = (F - kpl * e - kdl * (v - vp)) / LD(mass)
        acc[2] -= LD(g)
        qe = _qmul(qp, np.array([q[0], -q[1], -q[2], -q[3]], LD))
        qe = -qe if qe[0] < 0 else qe
        tau = tp - np.cross(e, F) + kpa * 2 * qe[1:] + kda * (wp - R @ wb)
        wd = Ii @ (R.T @ tau - np.cross(wb, Ib @ wb))
        return np.concatenate([v, acc, _qmul(q, np.array([0, *wb], LD)) / 2, wd])
    for k in range(len(rows37) - 1):
        rp, vp, qp, wp, F, tp = _plan_row(rows37[k])
        for _ in range(per_tick):
            k1 = f(y); k2 = f(y + h / 2 * k1); k3 = f(y + h / 2 * k2); k4 = f(y + h * k3)
            y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
            y[6:10] /= np.sqrt(y[6:10] @ y[6:10])
    return y


def test_the_rule_is_a_first_order_method_against_an_rk4_of_its_own():
    """400 ticks at 200 Hz of the exp_5 step plan (the base pitches) with moderate gains and the physical inertia: the rule's error
    in r and in q against a longdouble RK4 (16 steps per tick, the same zero-order hold, the oracle's rows, its own quaternion
    algebra) at substeps 1, 2, 4, 8: successive ratios in 1.5 .. 2.5."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan("exp5")
    hz, n = 200.0, 401
    c = plan.O.sample(plan.x, 0.25, hz, n)
    assert np.abs(c[:, 5]).max() > 1e-2
    want = rk4_rollout(c, hz, plan.cfg.mass, plan.cfg.gravity, INERTIA_PHYSICAL, rc.GAINS)
    wq = np.array([want[7], want[8], want[9], want[6]], LD)
    err_r, err_q = {}, {}
    for sub in (1, 2, 4, 8):
        p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, substeps=sub, **rc.GAINS)
        _, rows, status, state, _, word = ro.rollout_rows(plan.L, plan.x, 0.25, hz, 0, n, p, dtype=LD)
        assert word == 0 and not (status & ~ro.GIMBAL).any()
        err_r[sub] = float(np.abs(rows[-1, 1:4] - want[0:3]).max())
        err_q[sub] = float(min(np.abs(rows[-1, 13:17] - wq).max(), np.abs(rows[-1, 13:17] + wq).max()))
    rc.record("cpu_order", dict(err_r=err_r, err_q=err_q))
    for err in (err_r, err_q):
        for a, b in ((1, 2), (2, 4), (4, 8)):
            assert 1.5 <= err[a] / err[b] <= 2.5, (err_r, err_q)


@pytest.mark.parametrize("m", [1, TILE, 299])
def test_two_segments_with_the_carried_state_are_one_call(m):
    """Rows [0, n) in one call equal [0, m) then [m, n) with the carried state, count and word, to the bit, in both dtypes."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan("walk")
    n = 300
    p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, substeps=2, f_fb_max=10.0, push_from=240, push_ticks=30, dev_max=0.042,
                         **rc.GAINS)
    kw = dict(mass_scale=1.3, push=(40.0, -20.0, 10.0, 0.1, 0.2, -0.1))
    for dt in (F64, LD):
        one = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 7, n, p, count=5, dtype=dt, **kw)
        a = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 7, m, p, count=5, dtype=dt, **kw)
        b = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 7 + m, n - m, p, state=a[3], count=a[4], word=a[5], dtype=dt, **kw)
        for i in range(3):
            assert same(np.concatenate([a[i], b[i]]), one[i])
        assert same(b[3], one[3]) and (b[4], b[5]) == (one[4], one[5]) == (5 + n, ro.FALLEN)
        st = one[2]
        assert (st & ro.CLIPPED).any() and (st & ro.PUSH).any() and 235 < int(np.argmax(st & ro.FALLEN)) < 265 and not st[0]


def test_fallen_and_non_finite_freeze_the_state():
    """dev_max 1e-3 and a push: bit 0 appears at the first row over the bound and stays, and the state is frozen bit for bit.  A NaN
    among the force nodes (of a body held on its plan by the gains) becomes a NaN force at some row, a NaN velocity at the next: bit
    1 from there on, likewise."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan("walk")
    n = 400
    p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, dev_max=1e-3, push_from=50, push_ticks=100)
    held = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, **rc.GAINS)
    for dt in (F64, LD):
        meas, rows, st, state, count, word = ro.rollout_rows(plan.L, plan.x, 0.0, 1000.0, 0, n, p, push=(6.0, 0, 0, 0, 0, 0), dtype=dt)
        k = int(np.argmax(rows[:, 17] > dt(1e-3)))
        assert 50 < k < 150 and (rows[:k, 17] <= dt(1e-3)).all()
        assert ((st & ro.FALLEN) != 0).tolist() == [False] * k + [True] * (n - k) and word == ro.FALLEN and count == n
        for cols in (slice(1, 4), slice(7, 17)):
            assert (rows[k:, cols] == rows[k, cols]).all()
        assert (meas[k:, 0:3] == meas[k, 0:3]).all() and (rows[k:, 19] == 0).all() and not (st[k:] & (ro.PUSH | ro.CLIPPED)).any()
        assert same(state, np.concatenate([rows[k, 1:4], rows[k, 7:10], rows[k, 13:17], state[10:13]]))
        S = plan.L.splines[6]
        var = int(np.asarray(S.idx).reshape(S.n_polys + 1, 2, 3)[:, 0, 2].max())          # a force node's z value of foot 0
        x = np.array(plan.x)
        x[var] = np.nan
        meas, rows, st, state, count, word = ro.rollout_rows(plan.L, x, 0.0, 200.0, 0, 1001, held, dtype=dt)
        bad = (st & ro.NONFINITE) != 0
        k = int(np.argmax(bad))
        assert 0 < k < 1000 and bad[k:].all() and not bad[:k].any() and word == ro.NONFINITE
        assert np.isfinite(rows[:k, 1:17]).all() and np.isnan(rows[k, 9]) and np.isfinite(rows[k, 1:3]).all()
        assert same(rows[k:, 1:17], np.tile(rows[k, 1:17], (1001 - k, 1)))


@pytest.mark.parametrize("sub", [1, 3])
@pytest.mark.parametrize("name", ["walk", "exp5"])
def test_the_kernel_tests_gains_clip_some_rows_and_leave_few_near_the_limit(name, sub):
    """What tests/test_gpu_rollout.py asks of its "held" case, in the statement alone: with rollout_cases' gains, the 9.5 N limit
    and window 2's extra weight (0.3 m g = 8.8 N) and push, the clip acts on some of window 2's rows and not on all, the body does
    not fall, and the rows on which bit 3 may differ between the kernel and the rule -- where a component lies within NEAR of its
    limit, found by scaling the limit by 1 -+ NEAR -- are at most 1 % of a window's rows.  On the oracle's plans (the walk is the
    plan the kernel test runs; its exp_5 plan is the device planner's of the same start and goal)."""
    from qtos_amd import rollout as ro
    plan = rc.plan(name)
    for b in (1, 2):
        n = int(rc.COUNTS[b])
        at, lo, hi = (rc.window_statement(plan.L, plan.cfg, plan.x, "held", sub, b, LD, scale=s) for s in (1.0, 1 - rc.NEAR, 1 + rc.NEAR))
        clipped = (at[2] & ro.CLIPPED) != 0
        assert clipped.sum() < n and (b == 1 or clipped.sum() > 0), clipped.sum()
        assert at[5] == 0 and not (at[2] & (ro.FALLEN | ro.NONFINITE | ro.GIMBAL)).any()
        near = rc.near_the_limit(lo[2], hi[2])
        assert near.sum() <= n // 100, np.nonzero(near)[0]
        assert np.array_equal(at[2] & ~ro.CLIPPED, lo[2] & ~ro.CLIPPED) and np.array_equal(at[2] & ~ro.CLIPPED, hi[2] & ~ro.CLIPPED)


def test_a_pending_window_is_set_on_its_plan_by_its_first_call_with_rows():
    """PENDING in the carried word: a call without rows keeps the state and the bit; the first call with rows gives the rows of
    an INIT call to the bit and clears it; no row's status carries it."""
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    plan = rc.plan("walk")
    p = ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, substeps=2, **rc.GAINS)
    for dt in (F64, LD):
        junk = np.full(13, 0.25).astype(dt)
        kept = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 40, 0, p, state=junk, count=3, word=ro.PENDING, dtype=dt)
        assert same(kept[3], junk) and (kept[4], kept[5]) == (3, ro.PENDING)
        got = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 40, 30, p, state=kept[3], count=kept[4], word=kept[5], dtype=dt)
        want = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 40, 30, p, count=3, dtype=dt)
        for i in range(4):
            assert same(got[i], want[i])
        assert (got[4], got[5]) == (want[4], want[5]) == (33, 0) and not (got[2] & ro.PENDING).any()
        on = ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 70, 5, p, state=got[3], count=got[4], word=got[5], dtype=dt)
        assert not same(on[1][0, 1:4], ro.rollout_rows(plan.L, plan.x, 0.25, 200.0, 70, 5, p, dtype=dt)[1][0, 1:4])      # carried, not set anew


def test_rollout_params():
    from qtos_amd import capi, rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL, PlannerConfig
    cfg = PlannerConfig.reference_compat()
    for inertia in (None, INERTIA_PHYSICAL, ((2.0, 0.3, 0.1), (0.3, 1.0, -0.2), (0.1, -0.2, 3.0))):
        g = capi.rollout_params(cfg=cfg, inertia_b=inertia, kp_lin=(1, 2, 3), substeps=3, hz=200.0, init=True, quaternion=True)
        Ib, Ii = np.array(g.inertia_b).reshape(3, 3), np.array(g.inertia_b_inv).reshape(3, 3)
        assert np.array_equal(Ib, np.asarray(cfg.inertia_b if inertia is None else inertia, F64))
        scale = np.abs(Ii) @ np.abs(Ib)                                                # an entry of the product is a sum of three products
        assert (np.abs(Ii @ Ib - np.eye(3)) <= 4 * U * np.maximum(scale, 1.0)).all()
        assert (g.mass, g.gravity, g.substeps, g.flags) == (cfg.mass, cfg.gravity, 3, capi.ROLLOUT_INIT | capi.ROLLOUT_QUAT)
        assert list(g.kp_lin) == [1.0, 2.0, 3.0] and list(g.kd_ang) == [0.0] * 3
    for bad in (np.zeros((3, 3)), ((1.0, 2.0, 3.0), (2.0, 4.0, 6.0), (0.0, 0.0, 1.0)), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            capi.rollout_params(cfg=cfg, inertia_b=bad)
        with pytest.raises(ValueError):
            ro.RolloutParams(cfg, inertia_b=bad)
    with pytest.raises(ValueError):
        capi.rollout_params(cfg=cfg, substeps=0)
