"""The create-time KKT self-test on the MI355X (pytest -m gpu): qtos_planner_selftest reports what the debug entry points give
for the same inputs, a checked create rejects the elimination order that loses digits and falls back to one that does not,
admits rule 0 where it is sound, passes at the first attempt on random transcriptions, and leaves no trace on the handle."""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _order(rule):
    """QTOS_ORDER for the planners created inside (None: unset)."""
    old = os.environ.get("QTOS_ORDER")
    if rule is None:
        os.environ.pop("QTOS_ORDER", None)
    else:
        os.environ["QTOS_ORDER"] = str(rule)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("QTOS_ORDER", None)
        else:
            os.environ["QTOS_ORDER"] = old


def _short(gait):
    from qtos_amd.config import PlannerConfig
    return PlannerConfig(gait=gait, duration=2.5, dt_base=0.05, dt_dynamic=0.05)


def _goals(cfg, B, seed):
    """flat_goals with the distance scaled to the horizon (as the accuracy test of tests/test_gpu_kernels.py scales them)."""
    from qtos_amd import workloads
    s, g = workloads.flat_goals(B, seed=seed)
    g[:, 0] = s[:, 0] + (g[:, 0] - s[:, 0]) * (cfg.duration / 5.0)
    return s, g


@pytest.mark.parametrize("gait", ["trot", "walk"])
@pytest.mark.parametrize("seed", [0, 2026])
def test_selftest_reports_what_the_debug_entry_points_give(gait, seed):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.knots100(gait=gait)
    with _order(None):
        P = capi.Planner(cfg, max_batch=2)
    try:
        t = P.selftest(seed)
        s, g = capi.selftest_problem(cfg)
        start, goal = np.stack([s, s]), np.stack([g, g])
        ins = [capi.selftest_inputs(cfg, seed, b) for b in range(2)]
        x = P.initial_guess(start, goal) + np.stack([i[0] for i in ins])
        P.debug_newton(start, goal, x, np.stack([i[1] for i in ins]), np.stack([i[2] for i in ins]))
        _, res = P.debug_residual(2, refine=False)
        _, res2 = P.debug_residual(2, refine=True)
        v = np.abs(np.stack([P.factor(b)[0] for b in range(2)])[:, :, 1:, :])
        stage = int(np.unravel_index(int(np.argmax(v)), v.shape)[1])
        print("[selftest %s seed %d] residual %.3e refined %.3e max |V| %.6e stage %d, %.2f ms" %
              (gait, seed, t.residual, t.residual_refined, t.max_factor, t.worst_stage, 1e3 * t.seconds))
        assert (t.order_rule, t.front, t.n_stages, t.n_problems) == (P.dims.order_rule, P.dims.front, P.dims.n_stages, 2)
        assert t.residual == res.max() and t.residual_refined == res2.max()          # same kernels, same inputs: the last bit
        assert t.max_factor == v.max() and t.worst_stage == stage
        assert t.growth_limit == 1.05 / cfg.eps_dual and t.tol_residual == 1e-6
        assert t.passed == 1 and t.residual < 1e-6 and t.residual_refined < 1e-11 and t.max_factor <= t.growth_limit
        again = P.selftest(seed)
        assert (again.residual, again.residual_refined, again.max_factor, again.worst_stage) == (t.residual, t.residual_refined, t.max_factor, t.worst_stage)
        assert P.selftest(seed, tol_residual=1e-30).passed == 0                        # (the tolerance is the caller's)
    finally:
        P.close()


def test_the_order_that_loses_digits_is_caught_at_create():
    """QTOS_ORDER=0 on the 2.5 s trot at 0.05 s knots: the finding of round 6 (residual 6.5e-3, factor entries 5.17e9 in stage 2);
    the bounds are those tests/test_gpu_kernels.py asserts for this case."""
    from qtos_amd import capi
    cfg = _short("trot")
    with _order(0):
        with pytest.raises(capi.SelftestError) as err:
            capi.Planner(cfg, max_batch=2, checked=True)
        a = err.value.attempts
        print("[caught] " + "; ".join("%s front %d refined %.2e" % (t.describe(), t.front, t.residual_refined) for t in a))
        assert len(a) == 1 and a[0].order_rule == 0 and a[0].passed == 0 and a[0].front == 80
        assert a[0].residual > 1e-4 and a[0].max_factor > 10.0 / cfg.eps_dual
        P = capi.Planner(cfg, max_batch=2)                  # the plain create under the same environment still returns a planner
        assert P.dims.order_rule == 0 and P.selftests == []
        P.close()


def test_fallback_to_the_next_candidate_gives_the_plain_planner():
    from qtos_amd import capi
    cfg = _short("trot")
    start, goal = _goals(cfg, 8, seed=5)
    with _order(None):
        P = capi.Planner(cfg, max_batch=8, checked=True, rules_mask=7)
        Q = capi.Planner(cfg, max_batch=8)
    try:
        a = P.selftests
        print("[fallback] " + "; ".join("%s front %d" % (t.describe(), t.front) for t in a))
        assert [(t.order_rule, t.front, t.passed) for t in a] == [(0, 80, 0), (2, 96, 1)]
        assert (P.dims.order_rule, P.dims.front) == (2, 96) == (Q.dims.order_rule, Q.dims.front)
        assert P.kkt_kernel() == Q.kkt_kernel() and P.env() == Q.env()
        for x, y in zip(P.plan(start, goal), Q.plan(start, goal)):
            assert np.array_equal(x, y)
    finally:
        P.close()
        Q.close()


def test_rule_0_is_admitted_under_guard_where_it_is_sound():
    """Walk 2.5 s at 0.05 s knots: rule 0 on 80 slots passes (the fuzz of round 6 recorded 3.0e-10) and is kept; its plans agree
    with those of the plain planner (rule 2, 96 slots) to the 1e-6 of the parity tests."""
    from qtos_amd import capi
    cfg = _short("walk")
    start, goal = _goals(cfg, 8, seed=5)
    with _order(None):
        P = capi.Planner(cfg, max_batch=8, checked=True, rules_mask=7)
        Q = capi.Planner(cfg, max_batch=8)
    try:
        a = P.selftests
        print("[rule 0 under guard] " + "; ".join("%s front %d" % (t.describe(), t.front) for t in a))
        assert len(a) == 1 and (a[0].order_rule, a[0].front, a[0].passed) == (0, 80, 1)
        assert (P.dims.order_rule, P.dims.front) == (0, 80) and (Q.dims.order_rule, Q.dims.front) == (2, 96)
        n0, s0, i0, v0 = P.plan(start, goal)
        n2, s2, i2, v2 = Q.plan(start, goal)
        gap = float(np.abs(n0 - n2).max())
        print("[rule 0 under guard] status %s / %s, iterations %s / %s, max |nodes(rule 0) - nodes(rule 2)| = %.3e" %
              (s0.tolist(), s2.tolist(), i0.tolist(), i2.tolist(), gap))
        assert (s0 == 0).all() and (s2 == 0).all()
        assert gap <= 1e-6, gap
    finally:
        P.close()
        Q.close()


def _property_cases():
    from qtos_amd.config import PlannerConfig
    rng = np.random.default_rng(2026)
    out = []
    for i in range(48):
        gait = ("walk", "trot")[int(rng.integers(0, 2))]
        duration = float(rng.integers(2, 57)) * 0.5
        dt = (0.05, 0.1, 0.2)[int(rng.integers(0, 3))]
        out.append((i, PlannerConfig(gait=gait, duration=duration, dt_base=dt, dt_dynamic=dt)))
    return out


def _is_lds_refusal(exc):
    return isinstance(exc, RuntimeError) and "(-4)" in str(exc)


def test_random_transcriptions_pass_at_the_first_attempt():
    """48 transcriptions (gait, duration 1 .. 28 s, knot spacing): those with a kernel instantiation for their front (208 slots at
    most) are created plain and checked; the checked create passes at the first attempt with the three bounds of the accuracy
    test and builds the planner the plain create builds.  A case is skipped only where BOTH creates refuse it for the LDS (-4),
    4 at most.  Skipped on the MI355X this was written on: 3 (cases 19, 22, 31: horizons of 17.5 .. 19 s at 0.05 s knots, whose
    evaluation kernels would need 156 .. 167 KB of LDS scratch); not passed at the first attempt: none (worst residual 8.9e-8)."""
    from qtos_amd import capi
    cases = _property_cases()
    kept, dropped = [], []
    with _order(None):
        for i, cfg in cases:
            d, _ = capi.analyze(cfg)
            (kept if d.front <= 208 else dropped).append((i, cfg, d.front))
        print("[property] dropped up front (no kernel instantiation): %s" % [(i, c.gait, c.duration, c.dt_base, f) for i, c, f in dropped])
        assert [i for i, _, _ in dropped] == [15] and dropped[0][2] == 224
        skipped, failed = [], []
        for i, cfg, front in kept:
            name = "case %d %s %.1f s dt %.2f" % (i, cfg.gait, cfg.duration, cfg.dt_base)
            plain = checked = None
            try:
                try:
                    plain = capi.Planner(cfg, max_batch=2)
                    dims_plain = (plain.dims.order_rule, plain.dims.front)
                    plain.close()                       # (one planner alive at a time)
                except RuntimeError as e:
                    plain, err_plain = None, e
                try:
                    checked = capi.Planner(cfg, max_batch=2, checked=True)
                except capi.SelftestError as e:
                    failed.append((name, [t.describe() for t in e.attempts]))
                    continue
                except RuntimeError as e:
                    assert plain is None and _is_lds_refusal(e) and _is_lds_refusal(err_plain), (name, e)
                    skipped.append(name)
                    continue
                assert plain is not None, (name, err_plain)
                a = checked.selftests
                print("[property] %s: %s, refined %.2e, front %d, %.2f ms" % (name, a[0].describe(), a[0].residual_refined, a[0].front, 1e3 * a[0].seconds))
                if not (len(a) == 1 and a[0].passed == 1 and a[0].residual < 1e-6 and a[0].residual_refined < 1e-11
                        and a[0].max_factor <= 1.05 / cfg.eps_dual):
                    failed.append((name, [t.describe() + " refined %.2e" % t.residual_refined for t in a]))
                assert (checked.dims.order_rule, checked.dims.front) == dims_plain or len(a) > 1, name
            finally:
                if checked is not None:
                    checked.close()
        print("[property] skipped (both creates -4): %s" % skipped)
        print("[property] not passed at the first attempt: %s" % failed)
        assert len(skipped) <= 4, skipped
        assert not failed, failed


def test_28_s_horizon_through_the_checked_local_planner():
    """exp_9's `-duration 28` (4.0 x tiles, the longest the reference sends) on flat ground."""
    from qtos_amd.planner import LocalPlanner
    args = {"-g": [2.5, 0.0, 0.24], "-s": [0.0, 0.0, 0.24], "-duration": 28.0}
    res = {}
    with _order(None):
        for checked in (False, True):
            lp = LocalPlanner(max_batch=1, checked=checked)
            try:
                st = lp.solve_batch([args], sample=False)
                P = lp.planner(28.0)
                res[checked] = (st, lp.last["nodes"].copy(), lp.last["iters"].copy(), [t.copy() for t in P.selftests], (P.dims.order_rule, P.dims.front))
            finally:
                lp.close()
    t = res[True][3]
    print("[28 s] status %s iterations %s; %s, front %d, %.2f ms" % (res[True][0], res[True][2].tolist(), t[0].describe(), t[0].front, 1e3 * t[0].seconds))
    assert res[False][3] == [] and len(t) == 1 and t[0].passed == 1 and t[0].n_problems == 2
    assert res[True][4] == res[False][4] == (t[0].order_rule, t[0].front)
    assert res[True][0] == res[False][0] and np.array_equal(res[True][1], res[False][1]) and np.array_equal(res[True][2], res[False][2])


def test_pool_of_checked_planners():
    from qtos_amd.config import PlannerConfig
    from qtos_amd.pool import PlannerPool
    with _order(None):
        plain = PlannerPool(PlannerConfig.knots100(gait="trot"), n_lanes=2, max_batch=4)
        pool = PlannerPool(PlannerConfig.knots100(gait="trot"), n_lanes=2, max_batch=4, checked=True)
    try:
        assert all(lane.P.selftests == [] for lane in plain.lanes)
        for lane in pool.lanes:
            assert len(lane.P.selftests) == 1 and lane.P.selftests[0].passed == 1
            assert lane.P.dims.order_rule == plain.lanes[0].P.dims.order_rule and lane.P.dims.front == plain.lanes[0].P.dims.front
    finally:
        plain.close()
        pool.close()


def test_selftest_leaves_no_trace_on_the_handle():
    import torch
    from qtos_amd import capi, workloads
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.knots100(gait="trot")
    B = 16
    ter = workloads.exp5_terrain()
    start, goal = workloads.step_goals(B, seed=4, terrain=ter)
    with _order(None):
        P, Q = capi.Planner(cfg, max_batch=B), capi.Planner(cfg, max_batch=B)
    try:
        for H in (P, Q):
            H.set_heightfields(ter[0], ter[1])          # (the self-test ignores the maps and must leave them)
        first = P.plan(start, goal)
        flat = capi.Planner(cfg, max_batch=2)
        t_flat = flat.selftest(3)
        flat.close()
        t = P.selftest(3)
        assert (t.residual, t.max_factor) == (t_flat.residual, t_flat.max_factor)        # flat ground whatever the handle carries
        second = P.plan(start, goal)
        never = Q.plan(start, goal)
        Q.plan(start, goal)
        for x, y, z in zip(first, second, never):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert P.totals() == Q.totals() and P.totals()[1] == 2 * int(first[2].sum())
        assert P.timing_detail()["pattern_calls"] == Q.timing_detail()["pattern_calls"]
        # between submit and wait: -5, as qtos_set_report
        dev = torch.device("cuda", 0)
        tin = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (start, goal)]
        out = (torch.empty((B, P.n), dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev))
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        P.submit(B, tin[0].data_ptr(), tin[1].data_ptr(), None, None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                 out[3].data_ptr(), st.cuda_stream)
        rc = P.lib.qtos_planner_selftest(P.h, 0, 0.0, capi.C.byref(capi.QtosSelftest()))
        P.wait()
        st.synchronize()
        assert rc == -5
        assert np.array_equal(out[0].cpu().numpy(), first[0]) and P.selftest(3).passed == 1
    finally:
        P.close()
        Q.close()


def test_checked_create_costs_no_more_than_half_a_plain_create_again():
    """The gate of the issue: a checked create whose first candidate passes takes at most 1.5 x the plain create measured right
    before it (the plain create is at least the host analysis; the self-test a handful of launches on two problems).  The
    medians of five creates each are in profiles/selftest_cost.json."""
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    cases = {"knots100 trot": PlannerConfig.knots100(gait="trot"), "knots100 walk": PlannerConfig.knots100(),
             "knots200": PlannerConfig.knots200(), "walk 28 s": PlannerConfig(gait="walk", duration=28.0)}
    with _order(None):
        capi.Planner(cases["knots100 trot"], max_batch=2).close()      # (the process's first create loads the code object)
        worst = []
        for name, cfg in cases.items():
            t0 = time.perf_counter()
            P = capi.Planner(cfg, max_batch=2)
            t1 = time.perf_counter()
            P.close()
            t2 = time.perf_counter()
            Q = capi.Planner(cfg, max_batch=2, checked=True)
            t3 = time.perf_counter()
            a = Q.selftests
            Q.close()
            print("[cost] %s: plain create %.1f ms, checked create %.1f ms (ratio %.3f), of which the self-test %.2f ms" %
                  (name, 1e3 * (t1 - t0), 1e3 * (t3 - t2), (t3 - t2) / (t1 - t0), 1e3 * a[0].seconds))
            assert len(a) == 1 and a[0].passed == 1
            worst.append(((t3 - t2) / (t1 - t0), name))
        assert max(worst)[0] <= 1.5, worst


def test_cli_selftest_prints_the_header_line(tmp_path, gv1):
    from qtos_amd import flags
    inp = gv1["inputs"]
    args = {"-g": inp["g"], "-s": inp["s"], "-s_ang": [0, 0, 0], "-e1": inp["ee"][0], "-e2": inp["ee"][1],
            "-e3": inp["ee"][2], "-e4": inp["ee"][3], "-t": 3.756, "-resolution": 0.01, "scripts": {}}
    argv = flags.cmd_args(args).split()
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("QTOS_ORDER", None)

    def run(extra, csv):
        cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "qtos_amd.main"] + argv + ["--out", str(csv)] + extra
        return subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=330)

    a = run(["--selftest", "--log", "-"], tmp_path / "a.csv")
    assert a.returncode == 0, a.stderr[-3000:]
    b = run(["--log", "-"], tmp_path / "b.csv")
    assert b.returncode == 0, b.stderr[-3000:]
    la, lb = a.stdout.splitlines(), b.stdout.splitlines()
    print("[cli] " + la[1])
    assert la[1].startswith("KKT self-test: rule ") and la[1].endswith(", passed") and ", residual " in la[1] and ", max |V| " in la[1]
    assert not any(ln.startswith("KKT self-test") for ln in lb)

    def untimed(lines):   # (the two timing lines are measured seconds)
        return [ln for ln in lines if "GPU secs" not in ln]
    assert untimed(la[:1] + la[2:]) == untimed(lb)
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()

def test_cli_exits_with_status_2_where_no_order_passes(tmp_path, monkeypatch, capsys):
    """The command-line twin on the transcription of the finding (QTOS_ORDER=0, trot 2.5 s at 0.05 s knots): the attempts are
    printed, no CSV is written, the exit status is 2."""
    from qtos_amd import main as cli
    from qtos_amd.planner import LocalPlanner
    monkeypatch.setenv("QTOS_ORDER", "0")
    monkeypatch.setattr(cli, "LocalPlanner", lambda **kw: LocalPlanner(cfg=_short("trot"), **kw))
    monkeypatch.chdir(tmp_path)
    rc = cli.main(["-g", "0.25", "0", "0.24", "--out", str(tmp_path / "c.csv"), "--selftest"])
    out = capsys.readouterr().out.splitlines()
    print("[cli] " + " | ".join(out))
    assert rc == 2 and out[0].startswith("KKT self-test: rule 0, residual ") and "rejected (stage " in out[0] and out[-1] == "status -> 2"
    assert not os.path.exists(tmp_path / "c.csv")
    assert cli.main(["-g", "0.25", "0", "0.24", "--out", str(tmp_path / "d.csv")]) == 0       # (without --selftest it plans, as today)
