"""The force QP's rule (qtos_amd/force_qp.py) without a GPU: the conditions on the cases of tests/force_qp_cases.py, the fit path to
the bit, a certificate of the limited path that is independent of the iteration, the exact optimum of two-stance rows by
enumeration of their active sets, the float64 floor the GPU gates are taken from, the summary's semantics, the argument errors
and what the limits cost on the plans.

Certificate.  A float64 table can hold the slack of an active row, mu_end / z = 1e-7 N and less next to forces of 10 N, to 1e-8 ..
1e-7 relative, whatever computed it.  So the gate of the stationarity residual |H x + q + G^T (mu_end / s)|inf is 8 x what the
LONGDOUBLE rule's forces attain once they are rounded to float64 -- the best float64 table there is -- and the float64 rule is
held to it.  Measured here: float64 rule 1.1e-6 N against 1.9e-7 N of the rounded longdouble rule on synth_trot (the largest ratio,
5.5), 1.5e-7 N against 6.8e-8 N on the walk; the figures of every case are in profiles/force_qp_accuracy.json under cpu_certificate_*."""
import numpy as np
import pytest

import force_qp_cases as qc
from force_qp_cases import F64, LD


@pytest.fixture(params=qc.NAMES)
def case(request):
    return qc.case(request.param)


def limited_rows(c, dtype=F64):
    out, q, st, D = c.rows(dtype)
    return np.nonzero(D["limited"])[0]


def test_the_cases_meet_their_conditions():
    from qtos_amd import force_qp as fq
    active = np.zeros(6, int)
    counts = set()
    for name in qc.NAMES:
        c = qc.case(name)
        out, q, st, D = c.rows(F64)
        cnt = D["stance"].sum(axis=1)
        share = D["limited"].sum() / max(int((cnt > 0).sum()), 1)
        assert share >= 0.05, (name, share)
        assert not (st & fq.CAP).any() and not (c.rows(LD)[2] & fq.CAP).any(), name
        _, band = qc.guard(c)
        assert band.mean() <= 0.01, (name, band.mean())
        act = D["stance"][:, :, None] & (D["slack"] <= c.qp.act_tol) & D["limited"][:, None, None]
        active += act.sum(axis=(0, 1))
        counts |= set(int(v) for v in cnt[act.any(axis=(1, 2))])
        print(name, "rows", c.n, "limited share %.3f" % share, "active per limit row", act.sum(axis=(0, 1)), "steps max", int(q[:, 0].max()))
    assert (active > 0).all(), active
    assert {2, 3, 4} <= counts, counts
    # the synthetic rows: every stance pattern on a limit
    seen = set()
    for name in ("synth_trot", "synth_walk"):
        D = qc.case(name).rows(F64)[3]
        seen |= set(tuple(int(v) for v in s) for s in D["stance"][D["limited"]])
    assert {(1, 0, 0, 1), (0, 1, 1, 0), (1, 1, 1, 1)} <= seen and any(sum(s) == 3 for s in seen), seen


def test_fit_path_rows_are_the_fits_rows_to_the_bit(case):
    from qtos_amd import force_fit as ff, force_qp as fq
    for dt in (F64, LD):
        out, q, st, D = case.rows(dt)
        want, wst = ff.fit_rows(case.L, case.x, qc.T0, case.hz, case.first, case.n, case.cfg, case.qp, terrain=case.terrain, dtype=dt)
        keep = ~D["limited"]
        assert keep.any() and np.array_equal(out[keep], want[keep]) and np.array_equal(st[keep] & 7, wst[keep] & 7)
        assert not (st[keep] & (fq.LIMITED | fq.CAP)).any() and (st[~keep] & fq.LIMITED).all()
        assert (q[keep][:, [0, 1, 2, 4, 5, 6]] == 0).all()
        sw = ~D["stance"]
        assert np.array_equal(out[:, 1:13].reshape(-1, 4, 3)[sw], np.asarray(D["f"])[sw])        # a swing foot: the plan's force, to the bit


def test_certificate_of_the_limited_rows(case):
    """From the forces alone, in longdouble: strictly feasible, stationary for the barrier at mu_end, within the duality gap."""
    o64, _, _, D64 = case.rows(F64)
    old, _, _, Dld = case.rows(LD)
    me = case.qp.mu_end
    rows = limited_rows(case)
    got, best, gaps = [], [], []
    for k in rows:
        P = qc.Dense(Dld, k, case.qp)
        s, r, gap = qc.certificate(P, P.x_of(o64[k, 1:13], Dld, k), me)
        sb, rb, _ = qc.certificate(P, P.x_of(np.asarray(old[k, 1:13], F64), Dld, k), me)          # the longdouble rule's forces, rounded
        assert s > 0 and sb > 0, (k, s, sb)
        got.append(r), best.append(rb), gaps.append((gap, P))
    gate = qc.MARGIN * max(best)
    qc.record("cpu_certificate_" + case.name, dict(rows=len(rows), stationarity_float64=max(got), stationarity_longdouble_rounded=max(best), gate=gate,
                                                   gap_over_bound=max(g / (6 * P.n * me) for g, P in gaps)))
    assert max(got) <= gate, (max(got), gate)
    for gap, P in gaps:
        extra = 0.5 * 3 * P.n * gate * gate * float(1.0 / (P.c * P.Winv.min()))                  # 1/2 r^T H^-1 r, H >= c W^-1
        assert gap <= 6 * P.n * me + extra, (gap, 6 * P.n * me, extra)


def test_two_stance_rows_against_the_optimum_by_enumeration():
    from qtos_amd import force_qp as fq
    done, worst = 0, 0.0
    for name in ("trot", "synth_trot", "ledge"):
        c = qc.case(name)
        o64, q, st, D = c.rows(F64)
        Dld = c.rows(LD)[3]
        rows = [k for k in limited_rows(c) if D["stance"][k].sum() == 2 and q[k, 7] > 0]
        for k in rows[:: max(len(rows) // 3, 1)][:3]:
            P = qc.Dense(Dld, k, c.qp)
            opt, found, spread = qc.enumerate_optimum(P)
            diff = float(P.objective(P.x_of(o64[k, 1:13], Dld, k)) - opt)
            print(name, "row", k, "objective - optimum %.3e" % diff, "bound %.3e" % (12 * c.qp.mu_end), "KKT points", found, "spread %.1e" % spread)
            assert 0 <= diff <= 12 * c.qp.mu_end * (1 + fq.CTOL), (name, k, diff)
            worst, done = max(worst, diff), done + 1
    assert done >= 8
    qc.record("cpu_enumeration", dict(rows=done, worst_over_optimum=worst))


def test_float64_rule_against_the_longdouble_rule(case):
    """The floor the GPU gates are taken from, per column group, outside the guard band."""
    band, inb = qc.guard(case)
    (o64, q64, s64, _), (old, qld, sld, _) = case.rows(F64), case.rows(LD)
    keep = ~inb
    assert np.array_equal(s64[keep], sld[keep]) and np.abs(q64[keep, 0] - qld[keep, 0]).max() <= 1
    fl = qc.floors(case, keep)
    qc.record("cpu_floor_" + case.name, dict(fl, band=band, in_band=int(inb.sum()), rows=case.n))
    assert fl["f_qp"] < 1e-6 and fl["slack"] < 1e-9                                                 # (a float64 statement of the same rule)
    if case.name == qc.NAMES[-1]:
        qc.record("cpu_floor_all_cases", qc.group_floors())


def test_summarise_and_accumulate_on_a_hand_made_table():
    from qtos_amd import force_qp as fq
    T, Q = np.zeros((5, 32)), np.zeros((5, 8))
    T[:, 13] = [0.1, -0.4, 0.4, 0.0, 0.2]
    T[:, 17] = [1.0, 2.0, np.nan, 0.5, 0.5]
    T[:, 19] = [3.0, 6.0, 1.0, 6.0, 0.0]
    Q[:, 5] = [0.0, 0.02, 0.0, 0.005, 0.02]
    s = fq.summarise(T, Q, 100, qc.TOL)
    assert list(s["max"]) == [0.4, np.inf, 6.0, 0.02] and list(s["row"]) == [101, 102, 101, 101] and list(s["count"]) == [4, 5, 2, 2]
    e = fq.summarise(T[:0], Q[:0], 7, qc.TOL)
    assert e.tobytes() == fq.empty_summary().tobytes() and list(e["row"]) == [-1] * 4 and (e["max"] == -np.inf).all()
    two = fq.accumulate(fq.accumulate(fq.empty_summary(), fq.summarise(T[:2], Q[:2], 100, qc.TOL)), fq.summarise(T[2:], Q[2:], 102, qc.TOL))
    assert two.tobytes() == s.tobytes()
    assert len(fq.report_lines(s, 1.0, 50.0, qc.TOL)) == 4 and "limited" in fq.report_lines(s)[3]


def test_argument_errors_of_qp_params():
    from qtos_amd import force_qp as fq
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.reference_compat()
    p = fq.qp_params(cfg)
    assert (p.mu, p.f_max, p.max_iter) == (cfg.friction, cfg.force_limit, 25) and p.mu_end > 0
    assert fq.qp_params(cfg, mu=0.2).f_max == cfg.force_limit and fq.qp_params(None, f_max=12.0).f_max == 12.0
    for kw in (dict(mu=0.0), dict(mu=-1.0), dict(f_max=0.0), dict(mu_end=0.0), dict(max_iter=0), dict(max_iter=26), dict(act_tol=float("nan")),
               dict(damping=0.0), dict(arm=0.0), dict(w_min=2.0), dict(mu=float("nan"))):
        with pytest.raises(ValueError):
            fq.qp_params(cfg, **kw)


def test_what_the_limits_cost_is_recorded():
    """Recorded, not gated: the residual wrench with limits against the fit's and the share of rows limited."""
    from qtos_amd import force_fit as ff, force_qp as fq
    entry = {}
    for name, plan, kw in (("trot_mu0.2", "trot", dict(mu=0.2)), ("trot_mu0.5", "trot", dict(mu=0.5)), ("walk_fmax12", "walk", dict(f_max=12.0))):
        P = qc.ffc.plan(plan)
        n = int(round(P.cfg.duration * qc.HZ)) + 1
        qp = fq.qp_params(P.cfg, **kw)
        out, q, st, D = fq.qp_rows(P.L, P.x, 0.0, qc.HZ, 0, n, P.cfg, qp, terrain=P.terrain, detail=True)
        fit = D["fit_rows"]
        entry[name] = dict(share_limited=float(D["limited"].mean()), res_lin_fit=float(np.abs(fit[:, 16:19]).max()), res_lin_qp=float(np.abs(out[:, 16:19]).max()),
                           res_ang_fit=float(np.abs(fit[:, 13:16]).max()), res_ang_qp=float(np.abs(out[:, 13:16]).max()),
                           moved=float(q[:, 5].max()), steps_max=int(q[:, 0].max()))
        assert (q[:, 6] >= 0).all() and np.isfinite(out).all()
    qc.record("cpu_cost_of_limits", entry)
