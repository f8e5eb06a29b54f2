"""Per-solve report in the layout of the Ipopt log the reference's ``./main`` prints (``logs/towr_log.out:40-85``).

The reference pipes the solver's stdout into ``logs/towr_log.out`` (scripts/main.py:50,91): problem dimensions, the
iteration table, the final measures, the evaluation counts, the ``EXIT:`` line and ``status -> N``.  This module formats
the same text from what the planner measures (``Planner.set_report`` / ``Planner.report``: the iteration history and the
final measures of ``k_report``, csrc/kernels.hpp).

What the columns mean here ("Per-solve report"):

* ``objective`` is 0: the planner solves a feasibility problem, as the reference's Ipopt does (its log prints 0 too).
* ``inf_pr`` the max violation of the working rows; ``inf_du`` max |Je'y + Ji'(z_u - z_l)| over the KKT system's unknowns;
  ``lg(mu)`` log10 of the barrier parameter; ``||d||`` the max norm of the step's direction; ``lg(rg)`` is ``-`` (no
  regularisation of the Hessian), as in the reference.
* ``alpha_du`` the step length of the bound multipliers z (the equality multipliers y come whole from the KKT solve);
  ``alpha_pr`` the primal step length, followed by the step kind in the slot Ipopt uses for its f / h tag:
  ``f`` a Newton step with a fresh factorisation, ``h`` a chord step (the stored factorisation with a new right-hand side),
  ``x`` a chord step that was discarded (alpha_pr 0, the iterate stays).  ``ls`` the number of line-search trials.
* The final block's overall NLP error is the max of the three measures: the objective is zero and Ipopt's scaling s_d is 1.
* The timing lines are the planner's own measured seconds of the call (HIP events), labelled as such: there is no
  CPU-seconds split into solver and function evaluations on a GPU.
"""
import math

# status -> EXIT line (the planner's status codes: 0 converged, 1 out of iterations / stalled / jammed, 2 numerical failure)
EXIT_LINES = {
    0: "EXIT: Optimal Solution Found.",
    1: "EXIT: Maximum Number of Iterations Exceeded.",
    2: "EXIT: Invalid number in NLP function or derivative detected.",
}
EXIT_STOPPED = "EXIT: Stopped without progress (stalled or jammed); the best iterate is returned."
KIND_TAGS = {0: "f", 1: "h", 2: "x"}

TABLE_HEADER = "iter    objective    inf_pr   inf_du lg(mu)  ||d||  lg(rg) alpha_du alpha_pr  ls"

_DIM_LABELS = (
    ("Number of nonzeros in equality constraint Jacobian...", "jac_nnz_eq"),
    ("Number of nonzeros in inequality constraint Jacobian.", "jac_nnz_ineq"),
    ("Number of nonzeros in Lagrangian Hessian.............", "hess_nnz"),
    None,
    ("Total number of variables............................", "n_vars_free"),
    ("                     variables with only lower bounds", "var_lower_only"),
    ("                variables with lower and upper bounds", "var_both"),
    ("                     variables with only upper bounds", "var_upper_only"),
    ("Total number of equality constraints.................", "n_eq"),
    ("Total number of inequality constraints...............", "n_ineq"),
    ("        inequality constraints with only lower bounds", "ineq_lower_only"),
    ("   inequality constraints with lower and upper bounds", "ineq_both"),
    ("        inequality constraints with only upper bounds", "ineq_upper_only"),
)


def dims_dict(dims, counts):
    """The header's numbers from QtosDims (capi.analyze / Planner.dims) and the Jacobian nonzeros of
    capi.analyze_counts (None: printed as 0)."""
    nz = counts or (0, 0)
    return dict(jac_nnz_eq=nz[0], jac_nnz_ineq=nz[1], hess_nnz=0, n_vars_free=dims.n_free, var_lower_only=0, var_both=0,
                var_upper_only=0, n_eq=dims.n_eq, n_ineq=dims.n_ineq, ineq_lower_only=dims.n_ineq_lower,
                ineq_both=dims.n_ineq_both, ineq_upper_only=dims.n_ineq_upper)


def header_lines(d):
    """The dimension block (towr_log.out:40-52) from a dict with the keys of dims_dict."""
    return ["" if e is None else "%s:%9d" % (e[0], d[e[1]]) for e in _DIM_LABELS]


def iteration_line(it, inf_pr, inf_du, mu, dnorm, alpha_du, alpha_pr, tag, ls, objective=0.0):
    """One row of the iteration table, in Ipopt's column format; tag is the one-character slot behind alpha_pr."""
    lg_mu = math.log10(mu) if mu > 0 else -99.0
    return "%4d  %13.7e %7.2e %7.2e %5.1f %7.2e %4s  %7.2e %7.2e%s%3d" % (
        it, objective, inf_pr, inf_du, lg_mu, dnorm, "-", alpha_du, alpha_pr, tag, ls)


def table_lines(rows):
    """Header and one line per history record (capi.HIST_NAMES columns; row 0 has the blank tag)."""
    out = [TABLE_HEADER]
    for i, r in enumerate(rows):
        inf_du = r[9] if r[9] == r[9] else float("nan")
        out.append(iteration_line(i, r[0], inf_du, r[2], r[3], r[5], r[4], " " if i == 0 else KIND_TAGS.get(int(r[7]), "?"),
                                  int(r[6])))
    return out


def final_lines(iterations, viol, inf_du, compl, err, n_con_evals, n_jac_evals, seconds=None, n_factorizations=None,
                n_chord_solves=None):
    """The block behind the table (towr_log.out:64-82): measures, evaluation counts and the timing lines.  seconds:
    (the call's measured seconds, of those in KKT solves) or None; the factorisation / chord-solve counts are printed
    when given."""
    def m(name, v):
        return "%s:   %22.16e    %22.16e" % (name, v, v)
    out = ["Number of Iterations....: %d" % iterations, "",
           "                                   (scaled)                 (unscaled)",
           m("Objective...............", 0.0),
           m("Dual infeasibility......", inf_du),
           m("Constraint violation....", viol),
           m("Complementarity.........", compl),
           m("Overall NLP error.......", err), "", ""]
    counts = (("objective function evaluations            ", n_con_evals),
              ("objective gradient evaluations            ", n_jac_evals),
              ("equality constraint evaluations           ", n_con_evals),
              ("inequality constraint evaluations         ", n_con_evals),
              ("equality constraint Jacobian evaluations  ", n_jac_evals),
              ("inequality constraint Jacobian evaluations", n_jac_evals),
              ("Lagrangian Hessian evaluations            ", 0))
    out += ["Number of %s = %d" % (k, v) for k, v in counts]
    if n_factorizations is not None:
        out.append("Number of KKT factorizations (planner)               = %d" % n_factorizations)
    if n_chord_solves is not None:
        out.append("Number of chord solves (planner)                     = %d" % n_chord_solves)
    if seconds is not None:
        out.append("Total GPU secs of the call (planner, measured)       = %10.3f" % seconds[0])
        out.append("GPU secs in KKT solves (planner, measured)           = %10.3f" % seconds[1])
    return out


def exit_line(status, iterations, max_iter):
    if status == 1 and iterations < max_iter:
        return EXIT_STOPPED
    return EXIT_LINES.get(int(status), "EXIT: Unknown status %d." % int(status))


def selftest_line(t):
    """The header's line on the create-time KKT self-test the planner passed (a capi.QtosSelftest)."""
    return "KKT self-test: rule %d, residual %.1e, max |V| %.2e, %s" % (t.order_rule, t.residual, t.max_factor,
                                                                        "passed" if t.passed else "rejected")


def format_report(dims, counts, rep, rows, max_iter, seconds=None, selftests=None):
    """The whole report of one solve: dims (QtosDims), counts (capi.analyze_counts), rep (capi.QtosReport), rows (its
    history), seconds (see final_lines), selftests (the attempts of a planner that was created checked: the one it runs
    is the last; None or empty: no line).  Ends with ``status -> N``."""
    lines = ["Per-solve report of the qtos_amd planner (interior point, HIP on gfx950)."]
    if selftests:
        lines.append(selftest_line(selftests[-1]))
    lines.append("")
    lines += header_lines(dims_dict(dims, counts)) + [""]
    lines += table_lines(rows) + [""]
    lines += final_lines(rep.iterations, rep.constraint_violation, rep.dual_infeasibility, rep.complementarity,
                         rep.nlp_error, rep.n_con_evals, rep.n_jac_evals, seconds, rep.n_factorizations,
                         rep.n_chord_solves)
    lines += ["", exit_line(rep.status, rep.iterations, max_iter), "status -> %d" % rep.status]
    return "\n".join(lines) + "\n"
