"""The rule of the rollout through the feet in numpy (qtos_amd/rollout_feet.py, what k_rollout_feet is held to) on the CPU: what it
shares with rollout.py to the bit, the identities of the damped weighted least-squares distribution, the limit, the carried state,
and what feedback through the feet does to the golden walk and the trot.  The plans and the gates: tests/rollout_feet_cases.py."""
import numpy as np
import pytest

import rollout_feet_cases as fc
from rollout_feet_cases import F64, LD, U

HELD = dict(substeps=2, dev_max=0.5, tilt_max=1.0, **fc.GAINS)


def params(plan, **kw):
    from qtos_amd import rollout as ro
    from qtos_amd.config import INERTIA_PHYSICAL
    return ro.RolloutParams(plan.cfg, inertia_b=INERTIA_PHYSICAL, **kw)


def run(plan, hz, first, n, p, feet=None, dt=F64, **kw):
    from qtos_amd import rollout_feet as rf
    return rf.rollout_feet_rows(plan.L, plan.x, 0.25, hz, first, n, p, feet, dtype=dt, detail=True, **kw)


@pytest.mark.parametrize("name", ["walk", "trot"])
def test_without_gains_r_and_v_are_the_free_wrench_rollouts_to_the_bit(name):
    """All gains 0, ff_scale 1, no limit, 300 rows at 1 kHz, substeps 2: rho~ = 0, so y = 0 and df = 0 exactly -- columns 13 .. 15 are
    0, f_a is the plan's force -- and r, v of every row are rollout.rollout_rows' to the bit, in float64 and in longdouble.  The
    torque is the same number formed another way (sum (p_e - r) x f_e against tau_p - e x F: only the lever's origin differs), so
    the rotation equals rollout.py's within 8 x the float64-vs-longdouble floor of q measured here."""
    from qtos_amd import rollout as ro
    plan = fc.plan(name)
    p = params(plan, substeps=2)
    got, want = {}, {}
    for dt in (F64, LD):
        got[dt] = run(plan, 1000.0, 40, 300, p, dt=dt)
        want[dt] = ro.rollout_rows(plan.L, plan.x, 0.25, 1000.0, 40, 300, p, dtype=dt)
        meas, rows, frows, st, state, count, word, det = got[dt]
        assert fc.same(rows[:, 0:4], want[dt][1][:, 0:4]) and fc.same(rows[:, 7:10], want[dt][1][:, 7:10]) and fc.same(meas[:, 0:3], want[dt][0][:, 0:3])
        assert fc.same(state[0:6], want[dt][3][0:6]) and (count, word) == (want[dt][4], want[dt][5])
        assert (frows[:, 13:16] == 0).all() and fc.same(frows[:, 0], rows[:, 0]) and (rows[:, 19] == 0).all()
        c37 = ro.plan_rows37(plan.L, plan.x, 0.25, 1000.0, 40, 300, dt)
        assert np.array_equal(frows[:, 1:13], c37[:, 25:37])
        assert np.array_equal(st & ~(64 | 128), want[dt][2])
    floor = max(fc.dist(got[F64][1][:, 13:17], got[LD][1][:, 13:17]), fc.dist(want[F64][1][:, 13:17], want[LD][1][:, 13:17]))
    apart = {str(np.dtype(dt)): fc.dist(got[dt][1][:, 13:17], want[dt][1][:, 13:17]) for dt in (F64, LD)}
    fc.record("cpu_gains0_%s" % name, dict(floor=floor, apart=apart))
    assert floor > 0 and max(apart.values()) <= 8 * floor, (apart, floor)


@pytest.mark.parametrize("name", ["walk", "trot", "flight"])
def test_identities_of_the_distribution(name):
    """Gains on, no limit, 200 Hz x 2 substeps (the flight schedule: its one second), a push in the middle.

    Damped least squares: M y = rho~ and what the feet deliver is (M - lambda I) y, so on every row with a stance foot
    |(dT / arm, dF)| = lambda |y|, lambda = damping n, with dT, dF the signed vectors behind columns 14 and 13.  Two point feet a, b:
    the delivered correction has no moment about the line through them, u . (tau_d - (p_a - r) x F_d) = 0 with u = (p_a - p_b) /
    |p_a - p_b|, whatever the gains asked for.  No stance foot: nothing is delivered, columns 13 and 14 are |F_fb| and |tau_fb| and
    bit 6 is set.
    Gates: 8 x the float64 floor of the quantity (its distance from the longdouble rule's on the same row), or the propagated
    bound if that is larger: the delivered wrench is a sum of at most 4 x 3 products of entries of M with y, each off by a few u, and
    y itself is off by cond(M) u |y|, which lambda |y| and the residual M y - rho~ both see as u |M| |y|: 64 u |M|_2 |y| per row, with
    |M|_2 = cond(M) lambda_min -- force_fit_cases' amplification by the condition number, no fixed cap.  For the moment about the
    line: 64 u max |l_e| sum |g_e|."""
    from qtos_amd import rollout_feet as rf
    plan = fc.plan(name)
    hz, n = (200.0, 801) if name != "flight" else (200.0, 201)
    p = params(plan, push_from=n // 2, push_ticks=40, **HELD)
    feet = rf.FeetParams(plan.cfg)
    push = (4.0, -2.0, 1.0, 0.05, 0.1, -0.05)
    out = {dt: run(plan, hz, 0, n, p, feet, dt, push=push) for dt in (F64, LD)}
    entry = {}
    det64 = out[F64][7]
    cnt = det64["stance"].sum(axis=1)
    alive = (out[F64][3] & 3) == 0
    assert alive.sum() > n // 2
    arm = feet.arm
    q = {}
    for dt in (F64, LD):
        meas, rows, frows, st, state, count, word, det = out[dt]
        lam = dt(F64(feet.damping)) * cnt.astype(dt)
        lhs = np.sqrt(((det["dT"] / dt(F64(arm))) ** 2).sum(axis=1) + (det["dF"] ** 2).sum(axis=1))
        rhs = lam * np.sqrt((det["y"] ** 2).sum(axis=1))
        tau_d, F_d = det["dT"] + det["tau_fb"], det["dF"] + det["F_fb"]
        line = np.zeros(n, dt)
        for j in np.nonzero(cnt == 2)[0]:
            a, b = np.nonzero(det["stance"][j])[0]
            u = det["lev"][j, a] - det["lev"][j, b]
            u = u / np.sqrt((u * u).sum())
            line[j] = (u * (tau_d[j] - np.cross(det["lev"][j, a], F_d[j]))).sum()
        q[dt] = dict(lhs=lhs, rhs=rhs, line=line)
        assert np.array_equal((st & rf.NO_STANCE) != 0, cnt == 0) and np.array_equal((st & rf.TWO_STANCE) != 0, cnt == 2) and not (st & rf.LIMITED).any()
        none = alive & (cnt == 0)
        assert fc.same(frows[none, 13], rows[none, 19]) and (frows[none, 15] == 0).all()
        assert np.array_equal(frows[none, 14], np.sqrt((det["tau_fb"][none] ** 2).sum(axis=1))) or \
            fc.dist(frows[none, 14], np.sqrt((det["tau_fb"][none] ** 2).sum(axis=1))) <= 4 * U
    some = alive & (cnt > 0)
    if name == "flight":
        assert (alive & (cnt == 0)).sum() >= 20 and (out[F64][2][alive & (cnt == 0), 13] > 0).any()
    normM = np.array([np.linalg.norm(np.asarray(det64["M"][j], F64), 2) for j in range(n)])
    normy = np.sqrt((np.asarray(det64["y"], F64) ** 2).sum(axis=1))
    K = fc.condition(det64["M"], some)
    bound = 64 * U * normM * normy
    floor = max(fc.dist(q[F64]["lhs"][some], q[LD]["lhs"][some]), fc.dist(q[F64]["rhs"][some], q[LD]["rhs"][some]))
    defect = {str(np.dtype(dt)): float(np.abs(q[dt]["lhs"] - q[dt]["rhs"])[some].max()) for dt in (F64, LD)}
    worst = float((np.abs(np.asarray(q[F64]["lhs"] - q[F64]["rhs"], F64)) - np.maximum(bound, 8 * floor))[some].max())
    entry["least_squares"] = dict(rows=int(some.sum()), cond=K, floor=floor, defect=defect, bound_max=float(bound[some].max()), over=worst)
    assert worst <= 0, entry
    assert float((np.abs(np.asarray(q[LD]["lhs"] - q[LD]["rhs"], F64)) - np.maximum(bound, 8 * floor))[some].max()) <= 0
    two = alive & (cnt == 2)
    if name == "trot":
        assert two.sum() > n // 2
    if two.any():
        lev = float(np.abs(np.asarray(det64["lev"], F64)[two]).max())
        g = np.asarray(out[F64][2][:, 15], F64)
        bound2 = 64 * U * lev * 2 * g
        floor2 = fc.dist(q[F64]["line"][two], q[LD]["line"][two])
        over = float((np.abs(np.asarray(q[F64]["line"], F64)) - np.maximum(bound2, 8 * floor2))[two].max())
        entry["two_feet"] = dict(rows=int(two.sum()), floor=floor2, moment=float(np.abs(np.asarray(q[F64]["line"], F64))[two].max()),
                                 asked=float(np.abs(np.asarray(det64["tau_fb"], F64))[two].max()), over=over)
        assert over <= 0, entry
        # ... while what the gains asked for does have a moment about that line: the feet leave it undelivered
        assert float(np.asarray(out[F64][2][two, 14], F64).max()) > 1e3 * float(np.maximum(bound2, 8 * floor2)[two].max())
    fc.record("cpu_identities_%s" % name, entry)


def test_the_limit_holds_exactly_and_its_bit_marks_the_rows_it_acted_on():
    """The golden walk at 200 Hz with the gains, a push of (4, 2, 0) N over the ticks 300 .. 499, mu 0.3 and f_max 25 N (the body stays
    up: with mu 0.5 and a push of (6, 3, 0) N it falls):
    with QTOS_FEET_LIMIT every stance force of columns 1 .. 12 obeys 0 <= f_z <= f_max and |f_x|, |f_y| <= mu f_z exactly (the
    limit is made of comparisons and one product, mu f_z, which the test forms the same way); bit 8 is set on exactly the rows where
    the unlimited force of a step -- formed again here from the row's y -- breaks a limit.  Recorded: the limit acts on 612 of the
    801 rows (float64), the first of them row 40, and not on the others."""
    from qtos_amd import rollout as ro, rollout_feet as rf
    plan = fc.plan("walk")
    hz, n = 200.0, 801
    p = params(plan, push_from=300, push_ticks=200, **dict(HELD, substeps=1))
    feet = rf.FeetParams(plan.cfg, mu=0.3, f_max=25.0, limit=True)
    push = (4.0, 2.0, 0.0, 0.0, 0.0, 0.0)
    counts = {}
    for dt in (F64, LD):
        meas, rows, frows, st, state, count, word, det = run(plan, hz, 0, n, p, feet, dt, push=push)
        assert word == 0
        f = frows[:, 1:13].reshape(n, 4, 3)
        on = det["stance"]
        mu, f_max = dt(F64(feet.mu)), dt(F64(feet.f_max))
        fz = f[:, :, 2]
        ok = (fz >= 0) & (fz <= f_max) & (np.abs(f[:, :, 0]) <= mu * fz) & (np.abs(f[:, :, 1]) <= mu * fz)
        assert ok[on].all()
        # the unlimited force of the (one) step of every tick, from y: where it breaks a limit, and only there, the bit is set
        ff = dt(F64(p.ff_scale))
        d = det["lev"] / dt(F64(feet.arm))
        acted = np.zeros(n, bool)
        plan_f = rf.plan_feet(plan.L, ro.plan_rows37(plan.L, plan.x, 0.25, hz, 0, n, dt), hz, 0, feet, dt)[1]
        for k in range(4):
            x = np.cross(det["y"][:, 0:3], d[:, k])
            raw = ff * plan_f[:, k] + (x + det["y"][:, 3:6]) * det["w"][:, k, None]
            z = np.minimum(np.maximum(raw[:, 2], 0), f_max)
            broke = (raw[:, 2] < 0) | (raw[:, 2] > f_max) | (np.abs(raw[:, 0]) > mu * z) | (np.abs(raw[:, 1]) > mu * z)
            acted |= broke & on[:, k]
        assert np.array_equal((st & rf.LIMITED) != 0, acted)
        counts[str(np.dtype(dt))] = int(acted.sum())
        assert 0 < acted.sum() < n and not acted[0]
        assert (frows[acted, 13] > 0).all()                                                # a limited row leaves something undelivered
    fc.record("cpu_limit_walk", dict(limited_rows=counts, rows=n))
    assert counts["float64"] == 612, counts


@pytest.mark.parametrize("m", [1, 256, 299])
def test_two_segments_with_the_carried_state_are_one_call(m):
    """Rows [0, n) in one call equal [0, m) then [m, n) with the carried state, count and word, to the bit, in both dtypes, with the
    limit on, a push and a body that falls on the way (the trot 1.1 x as heavy, dev_max 0.06 m: it falls at row 255, in the push)."""
    from qtos_amd import rollout as ro, rollout_feet as rf
    plan = fc.plan("trot")
    n = 300
    p = params(plan, substeps=2, f_fb_max=10.0, push_from=240, push_ticks=30, dev_max=0.06, **fc.GAINS)
    feet = rf.FeetParams(plan.cfg, limit=True)
    kw = dict(mass_scale=1.1, push=(40.0, -20.0, 10.0, 0.1, 0.2, -0.1))
    for dt in (F64, LD):
        one = run(plan, 200.0, 7, n, p, feet, dt, count=5, **kw)
        a = run(plan, 200.0, 7, m, p, feet, dt, count=5, **kw)
        b = run(plan, 200.0, 7 + m, n - m, p, feet, dt, state=a[4], count=a[5], word=a[6], **kw)
        for i in range(4):
            assert fc.same(np.concatenate([a[i], b[i]]), one[i])
        assert fc.same(b[4], one[4]) and (b[5], b[6]) == (one[5], one[6]) == (5 + n, ro.FALLEN)
        st = one[3]
        k = int(np.argmax(st & ro.FALLEN))
        assert (st & ro.PUSH).any() and (st & rf.LIMITED).any() and 235 < k < 265 and not st[0] & 31
        # the frozen rows: 0 in columns 13 .. 15, the plan's forces in 1 .. 12, no limit bit
        c37 = ro.plan_rows37(plan.L, plan.x, 0.25, 200.0, 7, n, dt)
        assert (one[2][k:, 13:16] == 0).all() and np.array_equal(one[2][k:, 1:13], c37[k:, 25:37]) and not (st[k:] & (rf.LIMITED | ro.PUSH | ro.CLIPPED)).any()
        assert ((st[k:] & rf.TWO_STANCE) != 0).any()


def test_a_pending_window_is_set_on_its_plan_by_its_first_call_with_rows():
    """PENDING in the carried word behaves as in rollout.py: a call without rows keeps state, count and word; the first call with
    rows gives the rows of an INIT call to the bit and clears the bit; no row's status carries it (bits 6 .. 8 are not it)."""
    from qtos_amd import rollout as ro, rollout_feet as rf
    plan = fc.plan("walk")
    p = params(plan, substeps=2, **fc.GAINS)
    feet = rf.FeetParams(plan.cfg, limit=True)
    for dt in (F64, LD):
        junk = np.full(13, 0.25).astype(dt)
        kept = run(plan, 200.0, 40, 0, p, feet, dt, state=junk, count=3, word=ro.PENDING)
        assert fc.same(kept[4], junk) and (kept[5], kept[6]) == (3, ro.PENDING) and kept[2].shape == (0, 16)
        got = run(plan, 200.0, 40, 30, p, feet, dt, state=kept[4], count=kept[5], word=kept[6])
        want = run(plan, 200.0, 40, 30, p, feet, dt, count=3)
        for i in range(5):
            assert fc.same(got[i], want[i])
        assert (got[5], got[6]) == (want[5], want[6]) == (33, 0) and not (got[3] & ro.PENDING).any()
        on = run(plan, 200.0, 70, 5, p, feet, dt, state=got[4], count=got[5], word=got[6])
        assert not fc.same(on[1][0, 1:4], run(plan, 200.0, 70, 5, p, feet, dt)[1][0, 1:4])                  # carried, not set anew


def test_what_feedback_through_the_feet_does_to_the_walk_and_the_trot():
    """Recorded, not gated: 1 kHz over the horizon (5001 rows, one substep), rollout_cases.GAINS (kp_lin 300, kd_lin 30, kp_ang 30,
    kd_ang 1), config.INERTIA_PHYSICAL, no push, float64; the feet's arm 0.2, damping 1e-6, w_min 0.01 and the configuration's
    friction 0.5 and force limit 1000 N.  Largest tilt [rad], largest |e| [m], largest of columns 13 [N] and 14 [N m]:

                 free wrench (rollout.py)   through the feet, no limit            through the feet, QTOS_FEET_LIMIT
      walk       0.0526   0.0019            0.0526   0.0026   1.65   0.219        0.0526   0.0026   1.65   0.255   (268 rows limited)
      trot       0.0097   0.0131            0.0519   0.0185   9.14   1.44         1.55     0.484    196    50.5    (1140 rows limited)

    The walk is hardly changed: three or four feet deliver nearly all that the gains ask for, and the limit acts on a twentieth of the
    rows.  The trot stands on two feet for 4375 of its 5001 rows: through the feet its tilt is five times the free wrench's, because the
    moment about the line through the two feet is not delivered, and with the limit on it FALLS -- the friction pyramid takes away the
    horizontal forces that held it, and the tilt passes 1 rad (with tilt_max 1.0 the freeze would stop it there).  What is asserted is
    only that the figures are finite, that the two-stance count is the gait's, and the finding's direction: the unlimited trot tilts
    more than the free-wrench trot, and the limited trot more than 1 rad."""
    from qtos_amd import rollout as ro, rollout_feet as rf
    entry = {}
    for name in ("walk", "trot"):
        plan = fc.plan(name)
        p = params(plan, **fc.GAINS)
        free = ro.rollout_rows(plan.L, plan.x, 0.0, 1000.0, 0, 5001, p, dtype=F64)
        entry[name] = dict(free=dict(tilt=float(free[1][:, 18].max()), e=float(free[1][:, 17].max())))
        for limit in (False, True):
            meas, rows, frows, st, state, count, word = rf.rollout_feet_rows(plan.L, plan.x, 0.0, 1000.0, 0, 5001, p, rf.FeetParams(plan.cfg, limit=limit), dtype=F64)
            assert np.isfinite(rows).all() and np.isfinite(frows).all() and word == 0
            entry[name]["limit" if limit else "feet"] = dict(tilt=float(rows[:, 18].max()), e=float(rows[:, 17].max()), miss_f=float(frows[:, 13].max()),
                                                             miss_t=float(frows[:, 14].max()), limited=int(((st & rf.LIMITED) != 0).sum()),
                                                             two_stance=int(((st & rf.TWO_STANCE) != 0).sum()))
    fc.record("cpu_walk_and_trot", entry)
    assert entry["trot"]["feet"]["two_stance"] == 4375 and entry["walk"]["feet"]["limited"] == 0
    assert entry["trot"]["feet"]["tilt"] > entry["trot"]["free"]["tilt"] and entry["trot"]["limit"]["tilt"] > 1.0
