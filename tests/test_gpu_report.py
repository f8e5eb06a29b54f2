"""Per-solve report on the MI355X (pytest -m gpu): the report changes no plan, its history agrees with the trace, its
final measures agree with a float64 recomputation from the debug entry points, and the CLI gives the reference's log
layout back."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, start_vector

pytestmark = pytest.mark.gpu


def _workload(name):
    from qtos_amd import workloads
    from qtos_amd.config import PlannerConfig
    B, mid = 256, None
    if name == "trot":
        c = PlannerConfig.knots100(gait="trot"); ter = workloads.exp1_terrain(); start, goal = workloads.flat_goals(B, 3)
    elif name == "walk":
        c = PlannerConfig.reference_compat(); ter = None; start, goal = workloads.flat_goals(B, 0)
    else:
        c = PlannerConfig.knots100(); ter = workloads.mixed_terrains(); start, goal, mid = workloads.mixed_goals(B, seed=7, terrains=ter)
    return c, ter, start, goal, mid


def _record(name, text):
    print("[%s] %s" % (name, text))   # (the measured figures DESIGN.md section 4 quotes; pytest -s shows them)


@pytest.mark.parametrize("name", ["trot", "walk", "mixed"])
def test_report_changes_no_plan_and_its_history_is_the_trace(name):
    from qtos_amd.capi import Planner
    c, ter, start, goal, mid = _workload(name)
    P = Planner(c, max_batch=start.shape[0])
    try:
        if ter is not None:
            P.set_heightfields(ter[0], ter[1])
        off = P.plan(start, goal, map_id=mid)
        P.set_report(True)
        on = P.plan(start, goal, map_id=mid)
        P.set_report(False)
        for a, b in zip(off, on):
            assert np.array_equal(a, b)
        nodes, status, iters, viol = on
        errs = []
        for b in range(start.shape[0]):
            rep, rows = P.report(b)
            tr = P.trace(b)
            assert rep.status == status[b] and rep.iterations == iters[b] and rep.n_rows == iters[b] + 1 == rows.shape[0]
            # inf_pr, theta, alpha_pr, mu: the trace's columns bit for bit
            assert np.array_equal(rows[:, [0, 1, 4, 2]], tr[:, :4])
            if status[b] == 0:
                assert rows[-1, 0] == viol[b]
            assert np.isfinite(rows[:, [3, 5, 8, 9]]).all()
            assert rep.n_factorizations + rep.n_chord_solves == iters[b]
            assert rep.n_con_evals == 1 + int(rows[1:, 6].sum()) and rep.n_jac_evals == max(int(iters[b]), 1)
            m = [rep.constraint_violation, rep.dual_infeasibility, rep.complementarity, rep.nlp_error]
            assert np.isfinite(m).all() and rep.nlp_error == max(m[:3])
            if status[b] == 0:
                assert rep.constraint_violation <= c.tol
                errs.append(rep.nlp_error)
        _record("report_nlp_error.txt", "%s: %d converged, overall NLP error max %.3e median %.3e" %
                (name, len(errs), max(errs), float(np.median(errs))))
        # the reduced default system: the overall NLP error of the converged problems, bounded per workload at about 1.5
        # times what DESIGN.md section 4 records (max 1.4e-2 / 3.6e-2 / 0.89, medians 1.4e-2 / 2.2e-2 / 2.2e-2)
        bound_max, bound_median = {"trot": (2.2e-2, 2.2e-2), "walk": (5.5e-2, 3.3e-2), "mixed": (1.35, 3.3e-2)}[name]
        assert max(errs) < bound_max and float(np.median(errs)) < bound_median
        _recompute_inf_du(name, P, c, ter, mid, on)
    finally:
        P.close()


def _recompute_inf_du(name, P, c, ter, mid, on):
    """The report's dual infeasibility of a few problems of a product workload -- the reduced default system: B-spline
    coefficients and footholds are the unknowns -- against oracle/duals.py: the oracle's Jacobian at the returned nodes on the
    problem's own map, the basis Z of the unknowns, y, z_l, z_u of Planner.duals, under the gate of test_gpu_steps.py item 8.
    The problems: the converged one with the largest overall NLP error (the figure DESIGN.md section 4 quotes per workload), and
    three seeded others, one of them not converged where there is one."""
    import step_cases as stc
    from oracle import duals
    from oracle.oracle import Oracle, oracle_dict
    nodes, status, iters, viol = on
    B = nodes.shape[0]
    reps = [P.report(b)[0] for b in range(B)]
    s, zl, zu, y = P.duals(B)
    rk, vf, _ = P.structure()
    free = np.nonzero(vf != 0)[0]
    conv = np.nonzero(status == 0)[0]
    worst = int(conv[np.argmax([reps[b].nlp_error for b in conv])])
    rng = np.random.default_rng(5)
    rest = np.setdiff1d(np.arange(B), [worst])
    bad = np.setdiff1d(np.nonzero(status != 0)[0], [worst])
    picks = [worst] + ([int(rng.choice(bad))] if len(bad) else [])
    picks += [int(b) for b in rng.choice(np.setdiff1d(rest, picks), 4 - len(picks), replace=False)]
    assert c.reduce_base and c.reduce_swing and c.terrain_mode == 1
    entry, basis = {}, {}
    for b in picks:
        m = 0 if mid is None else int(mid[b])
        if ter is None:
            O = Oracle(oracle_dict(stc.lc.full(c)))
        else:
            O = Oracle(oracle_dict(stc.lc.full(c)), height=ter[0] if np.ndim(ter[0]) == 2 else ter[0][m], hcell=ter[1])
        if not basis:
            basis["Z"], basis["groups"] = duals.solver_basis(O, O.L, c, free)      # (the same on every map)
        assert not y[b][rk != 1].any() and not zl[b][rk != 2].any() and not zu[b][rk != 2].any()
        val, col, info = duals.dual_infeasibility(O.jacobian(nodes[b]), basis["Z"], y[b], zl[b], zu[b])
        gate = stc.dual_gate(info, stc.GATE_ENTRY)
        r = reps[b]
        entry[str(b)] = dict(status=int(status[b]), iterations=int(iters[b]), map=m, report_inf_du=r.dual_infeasibility, restated_inf_du=val, gate=gate,
                             achieved_over_bound=abs(r.dual_infeasibility - val) / gate, group=duals.GROUPS[basis["groups"][col]],
                             constraint_violation=r.constraint_violation, complementarity=r.complementarity, nlp_error=r.nlp_error,
                             largest_nlp_error_of_the_converged=b == worst)
    stc.record_dual("workloads", name, entry)
    for b, e in entry.items():
        assert abs(e["report_inf_du"] - e["restated_inf_du"]) <= e["gate"], (name, b, e)


def test_cold_start_of_the_logged_solve_prints_the_reference_first_row(cfg):
    from test_oracle_golden import GV3_INPUTS
    from qtos_amd import report
    from qtos_amd.capi import Planner
    P = Planner(cfg, max_batch=4)
    try:
        P.set_report(True)
        start, goal = start_vector(GV3_INPUTS)[None], np.array(GV3_INPUTS["g"])[None]
        nodes, status, iters, viol = P.plan(start, goal)
        rep, rows = P.report(0)
        lines = report.table_lines(rows)
        _record("report_gv3_table.txt", "\n".join(lines))
        assert status[0] == 0 and lines[1].split()[2] == "1.94e+01"   # logs/towr_log.out:56
        assert len(lines) == iters[0] + 2
    finally:
        P.close()


def test_final_measures_equal_a_float64_recomputation_on_the_full_system(cfg, oracle):
    """reduce_base = reduce_swing = 0: the KKT system's unknowns are the free nodes, so k_report's dual infeasibility
    and complementarity can be recomputed from qtos_debug_eval's dense Jacobian at the returned nodes and the state
    qtos_debug_duals hands back."""
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    B = 16
    P = Planner(dataclasses.replace(cfg, reduce_base=False, reduce_swing=False), max_batch=B)
    try:
        start, goal = workloads.flat_goals(B, seed=11)
        P.set_report(True)
        nodes, status, iters, viol = P.plan(start, goal)
        reps = [P.report(b)[0] for b in range(B)]
        s, zl, zu, y = P.duals(B)                       # (before debug_eval: that call reuses the workspace)
        rk, vf, _ = P.structure()
        lo, hi = oracle.con_bounds()
        _, J = P.debug_eval(start, goal, nodes)
        iq = rk == 2
        hl, hu = iq & (lo > -1e19), iq & (hi < 1e19)
        free = vf != 0
        worst = 0.0
        for b in range(B):
            assert np.all(y[b][rk != 1] == 0) and np.all(zl[b][~iq] == 0) and np.all(zu[b][~iq] == 0)
            v = y[b] + zu[b] - zl[b]
            Jf = J[b][:, free]
            du_terms = Jf.T @ v
            du = np.abs(du_terms).max()
            scale = (np.abs(Jf).T @ np.abs(v)).max()
            cp = max(np.abs((s[b] - lo) * zl[b])[hl].max(initial=0.0), np.abs((hi - s[b]) * zu[b])[hu].max(initial=0.0))
            r = reps[b]
            assert abs(r.complementarity - cp) <= 1e-9 * abs(cp)
            # (summation order: the device sums the same products in another order; bounded by the size of the terms)
            assert abs(r.dual_infeasibility - du) <= 1e-9 * abs(du) + 1e-15 * scale
            worst = max(worst, abs(r.dual_infeasibility - du) / max(abs(du), 1e-300))
        _record("report_recompute.txt", "full system, %d problems: worst relative difference of the dual infeasibility %.2e" % (B, worst))
    finally:
        P.close()


def test_set_report_is_refused_while_a_call_is_open(cfg):
    import torch
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    B = 4
    P = Planner(cfg, max_batch=B)
    try:
        start, goal = workloads.flat_goals(B, seed=2)
        dev = torch.device("cuda", 0)
        t = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (start, goal)]
        out = (torch.empty((B, P.n), dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float64, device=dev))
        st = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        P.submit(B, t[0].data_ptr(), t[1].data_ptr(), None, None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                 out[3].data_ptr(), st.cuda_stream)
        assert P.lib.qtos_set_report(P.h, 1) == -5
        P.wait()
        st.synchronize()
        assert P.lib.qtos_set_report(P.h, 1) == 0
        assert P.lib.qtos_set_report(P.h, 0) == 0
    finally:
        P.close()


def test_cli_log_to_stdout_gives_the_reference_layout_and_the_same_csv(tmp_path, gv1):
    from qtos_amd import flags
    inp = gv1["inputs"]
    args = {"-g": inp["g"], "-s": inp["s"], "-s_ang": [0, 0, 0], "-e1": inp["ee"][0], "-e2": inp["ee"][1],
            "-e3": inp["ee"][2], "-e4": inp["ee"][3], "-t": 3.756, "-resolution": 0.01, "scripts": {}}
    argv = flags.cmd_args(args).split()
    env = dict(os.environ, PYTHONPATH=ROOT)

    def run(extra, csv):
        cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "qtos_amd.main"] + argv + ["--out", str(csv)] + extra
        return subprocess.run(cmd, cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=330)

    a = run(["--log", "-"], tmp_path / "a.csv")
    assert a.returncode == 0, a.stderr[-3000:]
    _record("report_cli_stdout.txt", a.stdout)
    lines = a.stdout.splitlines()
    assert any(ln.startswith("Total number of variables............................:     1005") for ln in lines)
    assert "iter    objective    inf_pr   inf_du lg(mu)  ||d||  lg(rg) alpha_du alpha_pr  ls" in lines
    assert "EXIT: Optimal Solution Found." in lines and lines[-1] == "status -> 0"
    assert sum(ln == "status -> 0" for ln in lines) == 1
    b = run([], tmp_path / "b.csv")
    assert b.returncode == 0, b.stderr[-3000:]
    assert b.stdout == "status -> 0\n"
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
