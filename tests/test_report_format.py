"""Per-solve report, CPU side: the formatter reproduces the reference's solver log (logs/towr_log.out, committed as the
fixture tests/golden/towr_log_report.json by tests/golden/make_report_golden.py), the dimension header comes from the
product's own host analysis, and the ctypes layer still loads a library without the report's entry points."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "towr_log_report.json")


@pytest.fixture(scope="module")
def log():
    return json.load(open(FIX))


def test_iteration_table_reproduces_the_reference_log(log):
    from qtos_amd import report
    got = [report.TABLE_HEADER]
    for r in log["rows"]:
        got.append(report.iteration_line(r["iter"], r["inf_pr"], r["inf_du"], 10.0 ** r["lg_mu"], r["dnorm"], r["alpha_du"],
                                         r["alpha_pr"], r["tag"], r["ls"], r["objective"]))
    assert got == log["table_lines"]


def test_history_rows_map_to_table_tags():
    import numpy as np
    from qtos_amd import report
    rows = np.zeros((4, 10))
    rows[:, 2] = 0.1
    rows[1:, 7] = [0, 1, 2]
    rows[1:, 6] = [1, 1, 1]
    tags = [ln[-4] for ln in report.table_lines(rows)[1:]]
    assert tags == [" ", "f", "h", "x"]


def test_final_block_reproduces_the_reference_log_but_the_cpu_seconds(log):
    from qtos_amd import report
    f = log["final"]
    got = report.final_lines(f["iterations"], f["viol"], f["inf_du"], f["compl"], f["err"], f["n_con_evals"], f["n_jac_evals"])
    got += ["", report.exit_line(f["status"], f["iterations"], 24), "status -> %d" % f["status"]]
    want = [ln for ln in log["final_lines"] if not ln.startswith("Total CPU secs")]
    assert got == want
    assert report.exit_line(1, 24, 24) == "EXIT: Maximum Number of Iterations Exceeded."
    assert report.exit_line(1, 9, 24).startswith("EXIT: Stopped")
    assert report.exit_line(2, 3, 24).startswith("EXIT: Invalid number")


def test_timing_lines_are_labelled_as_the_planners_own():
    from qtos_amd import report
    lines = report.final_lines(3, 1e-5, 1e-3, 1e-4, 1e-3, 5, 3, seconds=(0.004, 0.002), n_factorizations=2, n_chord_solves=1)
    assert not any("CPU secs" in ln for ln in lines)
    assert any(ln.startswith("Total GPU secs of the call (planner, measured)") for ln in lines)
    assert "Number of KKT factorizations (planner)               = 2" in lines


def test_header_from_the_host_analysis_matches_the_reference_log(hip_lib, cfg, log):
    """Lines 40-52 of the log from qtos_analyze + qtos_analyze_counts.  Every line but the two Jacobian nonzero counts is
    the reference's byte for byte; those two are this transcription's stored entries (the next test)."""
    from qtos_amd import capi, report
    d, _ = capi.analyze(cfg)
    got = report.header_lines(report.dims_dict(d, capi.analyze_counts(cfg)))
    want = log["dims_lines"]
    assert len(got) == len(want) == 13
    assert got[2:] == want[2:]
    assert got[:2] == ["Number of nonzeros in equality constraint Jacobian...:    22017",
                       "Number of nonzeros in inequality constraint Jacobian.:    21597"]


def test_jacobian_nonzero_counts_are_the_stored_entries_of_the_blocks(hip_lib, cfg, oracle):
    """qtos_analyze_counts counts the entries of the model's Jacobian blocks over the free variables -- the structure the
    planner stores, as Ipopt's header counts the structure its NLP interface stores.  Pinned exactly; and no entry that
    is nonzero at a generic point lies outside it: the oracle's complex-step Jacobian of the same NLP at a perturbed
    starting point has fewer nonzeros in each row class.

    towr's 11557 / 20605 (tests/golden/nlp_dims.json) cannot be derived from the NLP: the same generic-point count gives
    10484 / 18905, so towr's figures include over a thousand entries per class that its own sparse assembly stores as
    zeros, and that code is not part of the reference tree."""
    import dataclasses
    import numpy as np
    from qtos_amd import capi, workloads
    counts = capi.analyze_counts(cfg)
    assert counts == (22017, 21597)
    full = capi.analyze_counts(dataclasses.replace(cfg, reduce_base=False, reduce_swing=False))
    assert full == counts                     # (counted on the full system whatever the reductions)
    start, goal = workloads.flat_goals(1, seed=3)
    s, g = start[0], goal[0]
    q = oracle.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), g)
    x0 = oracle.initial_guess(q)
    x = x0 + 0.05 * np.random.default_rng(0).standard_normal(x0.size)
    xl, xu = oracle.var_bounds(q)
    lo, hi = oracle.con_bounds()
    nz = (oracle.jacobian(x)[:, xl != xu] != 0).sum(axis=1)
    eq = lo == hi
    generic = (int(nz[eq].sum()), int(nz[~eq].sum()))
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "nlp_dims.json")))
    assert generic[0] <= counts[0] and generic[1] <= counts[1]
    assert generic[0] < golden["jac_nnz_eq"] and generic[1] < golden["jac_nnz_ineq"]


def test_capi_loads_a_library_without_the_report_entry_points(tmp_path, hip_lib):
    """A build from before the report (loaded through QTOS_LIB for A/B timing) still loads: the new prototypes are guarded."""
    from qtos_amd import capi
    new = {"qtos_set_report", "qtos_plan_report", "qtos_analyze_counts", "qtos_debug_duals"}
    src = tmp_path / "stub.c"
    src.write_text("".join("int %s(void) { return -1; }\n" % n for n in capi.EXPORTS if n not in new))
    so = tmp_path / "libstub.so"
    subprocess.check_call(["cc", "-shared", "-fPIC", "-o", str(so), str(src)])
    code = ("from qtos_amd import capi; from qtos_amd.config import PlannerConfig; lib = capi.load(); "
            "assert not hasattr(lib, 'qtos_set_report'); assert capi.analyze_counts(PlannerConfig.reference_compat()) is None; "
            "print('ok')")
    env = dict(os.environ, QTOS_LIB=str(so), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]
