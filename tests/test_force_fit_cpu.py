"""The force-fit rule in numpy (qtos_amd/force_fit.py, what k_force_fit is held to) on the three plans of
tests/test_plan_check_cpu.py and on a schedule with a flight phase, its summary's semantics, and the C ABI without a device.  The
plans, the gates and their derivation are in tests/force_fit_cases.py.

Measured here (float64 numpy, 5001 rows at 1 kHz, arm 0.2 m, damping 1e-6, w_min 0.01; profiles/force_fit_accuracy.json has
every figure):

  plan   stance feet  rows   lin before -> after      ang before -> after        largest |df|   fitted forces outside the pyramid
  trot   4             626   1.39 N  -> 4.0e-6 N      0.055 N m -> 6.3e-7 N m    0.61 N         0.012 N
  trot   2            4375   20.9 N  -> 0.58 N        0.20 N m  -> 0.084 N m     11.3 N         3e-7 N
  exp5   4            1848   2.47 N  -> 9.0e-6 N      0.51 N m  -> 1.3e-6 N m    1.86 N         0.008 N
  exp5   3            2913   1.54 N  -> 2.7e-4 N      0.40 N m  -> 3.6e-5 N m    1.69 N         0.005 N
  exp5   2             240   1.12 N  -> 0.52 N        0.24 N m  -> 0.070 N m     1.31 N         none
  walk   3            2913   1.52 N  -> 2.7e-4 N      0.43 N m  -> 3.6e-5 N m    1.68 N         0.025 N

The limit test.  The rule's weights are w_e = max(n max(g_e, 0) / sum max(g, 0), w_min): with w_min = 1 they are max(4 g_e / sum g, 1),
at least 1 and NOT all equal (up to 2.2 on these plans), so the fit's df is the solution of A~ df = rho~ of least weighted norm
sum |df_e|^2 / w_e, and differs from numpy.linalg.lstsq's plain minimum-norm solution by up to tenths of a newton (printed).  The
test therefore holds two things to lstsq within the gate: the rule's own solve (force_fit.system and cholesky_solve) with weights
that are all 1 against the plain minimum-norm solution, and fit_rows(w_min = 1, damping = 1e-12) against the minimum weighted-norm
solution, W^1/2 lstsq(A~ W^1/2, rho~) with the rule's weights."""
import ctypes as C

import numpy as np
import pytest

import force_fit_cases as ffc
from force_fit_cases import F64, LD

HZ, N = 1000.0, 5001


@pytest.fixture(params=["walk", "trot", "exp5"])
def plan(request):
    return ffc.plan(request.param)


_tables = {}


def tables(p, **kw):
    """(float64 table, status, detail), (longdouble ...) of a plan's 5001 rows, computed once per set of keywords."""
    from qtos_amd import force_fit as ff
    key = (p.name,) + tuple(sorted(kw.items()))
    if key not in _tables:
        fit = ff.fit_params(p.cfg, **{k: v for k, v in kw.items() if k != "mass_scale"})
        _tables[key] = tuple(ff.fit_rows(p.L, p.x, 0.0, HZ, 0, N, p.cfg, fit, terrain=p.terrain, mass_scale=kw.get("mass_scale", 1.0),
                                         dtype=dt, detail=True) for dt in (F64, LD))
    return _tables[key]


def test_residual_columns_are_the_dynamics_rows_of_the_fitted_forces(plan):
    """Columns 13 .. 18 (formed as rho - A df) against g_ang, g_lin formed anew from dyn_angular, m a + m g e_z and columns 1 .. 12."""
    from qtos_amd import plan_check as pc
    (t64, _, d64), (tld, _, _) = tables(plan)
    sp, x = plan.L.splines, np.asarray(plan.x)
    _, t = pc.row_times(plan.L, HZ, 0, N)
    r, a = pc.eval_spline(sp[0], x, t, 0, LD), pc.eval_spline(sp[0], x, t, 2, LD)
    th, thd, thdd = (pc.eval_spline(sp[1], x, t, k, LD) for k in range(3))
    m, g = LD(plan.cfg.mass), LD(plan.cfg.gravity)
    entry = {}
    for name, table in (("float64", t64), ("longdouble", tld)):
        g_ang = pc.dyn_angular(plan.cfg.inertia_b, th, thd, thdd, LD)
        g_lin = m * a
        g_lin[:, 2] += m * g
        for e in range(4):
            f = np.asarray(table[:, 1 + 3 * e:4 + 3 * e], LD)
            g_ang = g_ang - np.cross(f, r - pc.eval_spline(sp[2 + e], x, t, 0, LD))
            g_lin = g_lin - f
        want = np.array(tld)
        want[:, 13:16], want[:, 16:19] = g_ang, g_lin
        cmp = ffc.compare(table, want, t64 if name == "float64" else tld, d64, groups={k: ffc.GROUPS[k] for k in ("res_ang", "res_lin")})
        # (the floor of this comparison is the float64 table's own distance from the longdouble one)
        floor = ffc.compare(t64, tld, t64, d64, groups={k: ffc.GROUPS[k] for k in ("res_ang", "res_lin")})
        for c in cmp:
            for grp, w in cmp[c].items():
                w["floor"] = floor[c][grp]["err"]
                w["gate"] = ffc.gate(grp, w["floor"], w["cond"])
        entry[name] = cmp
        ffc.assert_within(cmp, name)
    ffc.record("cpu_consistency_" + plan.name, entry)


def test_the_residual_never_grows(plan):
    """|(res_ang / arm, res_lin)| <= |rho~| on every row with a stance foot: M >= damping n I."""
    (t64, _, d64), (tld, _, dld) = tables(plan)
    arm = 0.2
    cnt = d64["stance"].sum(axis=1)
    for table, D in ((t64, d64), (tld, dld)):
        before = np.sqrt(((np.asarray(D["rho"], LD) / np.r_[[arm] * 3, [1.0] * 3].astype(LD)) ** 2).sum(axis=1))
        after = np.sqrt((np.asarray(table[:, 13:16], LD) / LD(arm)) ** 2 @ np.ones(3, LD) + np.asarray(table[:, 16:19], LD) ** 2 @ np.ones(3, LD))
        for c in sorted(set(cnt[cnt > 0])):
            m = cnt == c
            slack = ffc.gate("res_lin", 0.0, ffc.condition(d64["M"], m)) + ffc.gate("res_ang", 0.0, ffc.condition(d64["M"], m)) / arm
            assert (after[m] <= before[m] + slack).all(), (c, float((after[m] - before[m]).max()))
    assert (cnt > 0).all()


def _lstsq_rows(D, rows, weighted):
    """The minimum (weighted-)norm solution of A~ df = rho~ per row, through numpy.linalg.lstsq in float64: [len(rows), 4, 3]."""
    out = np.zeros((len(rows), 4, 3))
    for i, k in enumerate(rows):
        d, w = np.asarray(D["d"][k], F64), (np.asarray(D["w"][k], F64) if weighted else np.ones(4))
        A = np.zeros((6, 12))
        for e in range(4):
            A[0:3, 3 * e:3 * e + 3] = np.array([[0, -d[e, 2], d[e, 1]], [d[e, 2], 0, -d[e, 0]], [-d[e, 1], d[e, 0], 0]])
            A[3:6, 3 * e:3 * e + 3] = np.eye(3)
        s = np.sqrt(np.repeat(w, 3))
        rho = np.asarray(D["rho"][k], F64) / np.r_[[0.2] * 3, [1.0] * 3]
        out[i] = (s * np.linalg.lstsq(A * s[None, :], rho, rcond=None)[0]).reshape(4, 3)
    return out


def test_the_limit_is_the_minimum_norm_solution(plan):
    from qtos_amd import force_fit as ff
    (t64, _, d64), (tld, _, dld) = tables(plan, w_min=1.0, damping=1e-12)
    four = np.nonzero(d64["stance"].all(axis=1))[0]
    assert len(four) >= 600
    rows = four[::7]                                                                   # (lstsq row by row: every seventh)
    m = np.zeros(N, bool)
    m[rows] = True
    K = ffc.condition(d64["M"], m)
    floor = ffc.dist(d64["df"][rows], dld["df"][rows])
    g = ffc.gate("f_fit", floor, K)
    # the rule's weights: the minimum weighted-norm solution
    weighted = _lstsq_rows(dld, rows, True)
    err_w = max(ffc.dist(d64["df"][rows], weighted), ffc.dist(dld["df"][rows], weighted))
    # all weights 1 through the rule's own solve: the plain minimum-norm solution
    ones = np.ones((N, 4), LD)
    lam = LD(1e-12) * LD(4) * np.ones(N, LD)
    M1 = ff.system(dld["d"], ones, dld["stance"], lam, LD)
    rho_s = np.concatenate([dld["rho"][:, 0:3] / LD(0.2), dld["rho"][:, 3:6]], axis=1)
    y = ff.cholesky_solve(M1[rows], rho_s[rows], LD)
    df1 = np.stack([np.cross(y[:, 0:3], dld["d"][rows, e]) + y[:, 3:6] for e in range(4)], axis=1)
    plain = _lstsq_rows(dld, rows, False)
    err_1 = ffc.dist(df1, plain)
    apart = ffc.dist(dld["df"][rows], plain)
    print("limit [%s]: weighted %.3g, equal weights %.3g, gate %.3g (cond %.3g, floor %.3g); the rule's weights reach %.3g and its df "
          "is %.3g N off the plain minimum-norm solution" % (plan.name, err_w, err_1, g, K, floor, float(dld["w"][rows].max()), apart))
    ffc.record("cpu_limit_" + plan.name, dict(weighted=err_w, equal_weights=err_1, gate=g, cond=K, floor=floor, rows=len(rows),
                                              w_max=float(dld["w"][rows].max()), off_plain_lstsq=apart))
    assert err_w <= g and err_1 <= g, (err_w, err_1, g)


def test_swing_feet_and_rows_without_stance_keep_the_plans_force(plan):
    from qtos_amd import force_fit as ff, plan_check as pc
    for p in (plan, ffc.plan("flight")):
        n = N if p is plan else 1001
        for dt in (F64, LD):
            if p is plan:
                table, status, D = tables(p)[0 if dt is F64 else 1]
            else:
                table, status, D = ff.fit_rows(p.L, p.x, 0.0, HZ, 0, n, p.cfg, terrain=p.terrain, dtype=dt, detail=True)
            _, t = pc.row_times(p.L, HZ, 0, n)
            cnt = D["stance"].sum(axis=1)
            assert np.array_equal((status & ff.NO_STANCE) != 0, cnt == 0) and np.array_equal((status & ff.TWO_STANCE) != 0, cnt == 2)
            assert not (status & ff.NONFINITE).any()
            for e in range(4):
                f = pc.eval_spline(p.L.splines[6 + e], np.asarray(p.x), t, 0, dt)
                sw = ~D["stance"][:, e]
                assert sw.any() and np.array_equal(table[sw, 1 + 3 * e:4 + 3 * e], f[sw])      # to the bit
                assert (np.abs(table[~sw, 1 + 3 * e:4 + 3 * e] - f[~sw]).max(axis=1) > 0).mean() > 0.9
            if p is not plan:
                none = cnt == 0
                assert none.sum() >= 150 and (status[none] == ff.NO_STANCE).all() and (table[none, 19] == 0).all()
                assert np.array_equal(table[none, 13:19], D["rho"][none])                           # nothing fitted: the plan's own rows
                assert (cnt[~none] == 4).all()


def test_mass_scale_scales_the_wrench_the_feet_supply(plan):
    (t64, _, d64), (tld, _, dld) = tables(plan, mass_scale=1.25)
    four = d64["stance"].all(axis=1)
    m, g = LD(plan.cfg.mass), LD(plan.cfg.gravity)
    for table, D in ((t64, d64), (tld, dld)):
        want = LD(1.25) * m * np.asarray(D["a"], LD)
        want[:, 2] += LD(1.25) * m * g
        total = sum(np.asarray(table[:, 1 + 3 * e:4 + 3 * e], LD) for e in range(4))
        off = np.abs(total - want)[four]
        res = np.abs(np.asarray(table[:, 16:19], LD))[four]
        slack = ffc.gate("res_lin", 0.0, ffc.condition(d64["M"], four))
        assert (off <= res + slack).all(), float((off - res).max())
        assert float(res.max()) < 1e-4 and float(np.abs(D["rho"][four, 3:6]).max()) > 5.0    # 7.4 N of weight the plan's forces lack


def test_feed_forward_columns(plan):
    from qtos_amd import force_fit as ff, joints
    n = 600
    jrows, _ = joints.joint_rows(plan.L, plan.x, 0.0, HZ, 2000, n, joints.JointParams(), dtype=F64)
    jrows = np.asarray(jrows, F64)
    out = {}
    for dt in (F64, LD):
        out[dt] = ff.fit_rows(plan.L, plan.x, 0.0, HZ, 2000, n, plan.cfg, terrain=plan.terrain, joint=jrows, dtype=dt, detail=True)
    (t64, _, d64), (tld, _, dld) = out[F64], out[LD]
    want = np.array(tld)
    for e in range(4):
        want[:, 20 + 3 * e:23 + 3 * e] = joints.feed_forward(e, jrows[:, 1 + 3 * e:4 + 3 * e], dld["th"], tld[:, 1 + 3 * e:4 + 3 * e], dtype=LD)
    cmp = ffc.compare(t64, want, t64, d64, groups={"tau": ffc.GROUPS["tau"]})
    for c in cmp:                                                                      # (the floor: the float64 f_fit's)
        K = cmp[c]["tau"]["cond"]
        cmp[c]["tau"]["gate"] = ffc.gate("tau", ffc.compare(t64, tld, t64, d64, groups={"f_fit": ffc.GROUPS["f_fit"]})[c]["f_fit"]["err"], K)
    ffc.assert_within(cmp)
    assert np.array_equal(tld[:, 20:32], want[:, 20:32]) and float(np.abs(want[:, 20:32]).max()) > 0.5
    plain = ff.fit_rows(plan.L, plan.x, 0.0, HZ, 2000, n, plan.cfg, terrain=plan.terrain, dtype=F64)[0]
    assert (plain[:, 20:32] == 0).all() and np.array_equal(plain[:, :20], t64[:, :20])


def test_summarise_semantics():
    from qtos_amd import force_fit as ff
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.reference_compat()
    n = 7
    T = np.zeros((n, ff.COLS))
    T[:, 3::3][:, :4] = 5.0                                                            # f_z = 5 N on every foot: inside the pyramid
    stance = np.ones((n, 4), bool)
    T[2, 13], T[5, 15] = -3.0, 3.0                                                     # a tie: the lowest row
    T[1, 16], T[3, 17] = 1e-2, 1e-2 + 1e-9                                             # count: strictly over tol
    T[4, 19] = np.nan                                                                  # non-finite: +inf
    T[6, 4] = 5.0 * cfg.friction + 0.25                                                # foot 1 pushes 0.25 N through the pyramid ...
    T[0, 7], stance[0, 2] = 9.0, False                                                 # ... a swing foot does not count
    T[3, 12] = np.nan                                                                  # a non-finite force of a stance foot: +inf
    s = ff.summarise(T, 100, stance, ffc.TOL, cfg)
    assert s.dtype == ff.SUMMARY and s.shape == (4,)
    assert (s["max"][0], s["row"][0], s["count"][0]) == (3.0, 102, 2)
    assert (s["max"][1], s["row"][1], s["count"][1]) == (1e-2 + 1e-9, 103, 1)
    assert (s["max"][2], s["row"][2], s["count"][2]) == (np.inf, 104, 1)
    assert (s["max"][3], s["row"][3], s["count"][3]) == (np.inf, 103, 2)
    T[3, 12] = 5.0
    s = ff.summarise(T, 100, stance, ffc.TOL, cfg)
    assert abs(s["max"][3] - 0.25) < 1e-12 and (s["row"][3], s["count"][3]) == (106, 1)
    empty = ff.summarise(np.zeros((0, ff.COLS)), 100, np.zeros((0, 4), bool), ffc.TOL, cfg)
    assert (empty["row"] == -1).all() and (empty["count"] == 0).all() and (empty["max"] == -np.inf).all()
    assert empty.tobytes() == ff.empty_summary().tobytes()
    # the accumulate rule on a real table: two parts against the whole, and merging nothing changes nothing
    p = ffc.plan("trot")
    table, _, D = tables(p)[0]
    table = np.array(table[:900])
    table[400, 14] = np.nan
    st = D["stance"][:900]
    whole = ff.summarise(table, 0, st, ffc.TOL, p.cfg)
    parts = ff.accumulate(ff.accumulate(ff.empty_summary(), ff.summarise(table[:333], 0, st[:333], ffc.TOL, p.cfg)),
                          ff.summarise(table[333:], 333, st[333:], ffc.TOL, p.cfg))
    assert parts.tobytes() == whole.tobytes() and whole["max"][0] == np.inf and whole["row"][0] == 400
    assert ff.accumulate(whole, empty).tobytes() == whole.tobytes()
    assert len(ff.report_lines(whole, 0.0, HZ, ffc.TOL)) == 4


def test_abi_exports_struct_and_argument_checks(hip_lib):
    from qtos_amd import capi, force_fit as ff
    for name in ("qtos_force_fit", "qtos_force_fit_device"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    assert capi.FIT_ACCUMULATE == ff.ACCUMULATE and capi.FIT_COLS == ff.COLS and capi.FIT_FAMILIES == len(ff.FAMILIES) == 4
    assert capi.FIT_TOL == ff.FIT_TOL
    assert C.sizeof(capi.QtosForceFit) == 8 + 4 + 4 + 8 + 8 + 4 * 8 + 4 * 8 + 12 * 8 + 4 * 8 + 2 * 8 + 4 * 8 + 8
    p = capi.fit_params(hz=0.0, n_rows=5, tol=1e-3, accumulate=True)
    assert list(p.tol) == [1e-3] * 4 and p.flags == 1 and p.first_row == 0 and p.capacity == 0 and capi.fit_params().flags == 0
    assert (p.arm, p.damping, p.w_min, p.excess_tol) == (0.2, 1e-6, 0.01, 1e-2)
    q = capi.fit_params(arm=0.3, damping=1e-4, w_min=1.0, excess_tol=0.5, capacity=7)
    assert (q.arm, q.damping, q.w_min, q.excess_tol, q.capacity) == (0.3, 1e-4, 1.0, 0.5, 7)
    j = capi.joint_params()
    assert list(p.lateral) == list(j.lateral) and (p.l_upper, p.l_lower, p.ee_shift) == (j.l_upper, j.l_lower, j.ee_shift)
    assert [list(h) for h in p.hip] == [list(h) for h in j.hip] and list(p.knee_sign) == list(j.knee_sign)
    for bad in (dict(arm=0.0), dict(arm=-1.0), dict(damping=0.0), dict(w_min=0.0), dict(w_min=1.5), dict(arm=float("nan"))):
        with pytest.raises(ValueError):
            ff.fit_params(None, **bad)
        with pytest.raises(ValueError):
            capi.fit_params(**bad)
    # a null planner answers -1 before anything touches a device (every other case leaves its reason in the handle: GPU tests)
    buf = np.zeros(64)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = buf.view(np.int32).ctypes.data_as(C.POINTER(C.c_int))
    assert hip_lib.qtos_force_fit(None, 1, C.byref(p), dp(buf), dp(buf), None, None, None, None, None, None, dp(buf), ip, None) == -1
    assert hip_lib.qtos_force_fit_device(None, 1, C.byref(p), buf.ctypes.data, buf.ctypes.data, None, None, None, None, None, None,
                                         buf.ctypes.data, buf.ctypes.data, None, None) == -1


def test_before_and_after_per_stance_count_are_recorded(plan):
    """Recorded, not gated: what the fit takes off the dynamics rows and what it costs, per stance count."""
    (t64, status, D), _ = tables(plan)
    cnt = D["stance"].sum(axis=1)
    entry = {}
    for c in sorted(set(int(v) for v in cnt)):
        m = cnt == c
        ex = np.where(D["stance"][m], D["excess"][m], -np.inf).max(axis=1)
        entry["stance_%d" % c] = dict(rows=int(m.sum()), lin_before=float(np.abs(D["rho"][m, 3:6]).max()), lin_after=float(np.abs(t64[m, 16:19]).max()),
                                      ang_before=float(np.abs(D["rho"][m, 0:3]).max()), ang_after=float(np.abs(t64[m, 13:16]).max()),
                                      df_max=float(np.abs(D["df"][m]).max()), change_max=float(t64[m, 19].max()), excess_max=float(ex.max()),
                                      cond=ffc.condition(D["M"], m), flagged=int(((status[m] >> 3) != 0).sum()))
    ffc.record("cpu_before_after_" + plan.name, entry)
    assert all(v["lin_after"] <= v["lin_before"] for v in entry.values())
