"""Command-line twin of the reference's ``./main``: same argv, same CSV, same exit status.

``args['scripts']['run']`` of the reference (QTOS/utils.py:17, 'docker exec <id> ./main') can be
pointed at ``python -m qtos_amd.main --out build/traj.csv`` unchanged otherwise.  ``--log PATH`` (``-``: stdout) writes
the per-solve report in the layout of the reference's ``logs/towr_log.out`` (report.py).  ``--selftest`` creates the planner
through the KKT self-test (capi.Planner(checked=True)): a transcription whose elimination orders all fail it is not planned --
the attempts are printed and the exit status is 2, the reference's "numerical failure" class.  ``--check`` prints, behind the
solve, what the plan violates between its knots: one line per family of the plan check (plan_check.py); the exit status is
unchanged.  ``--fit`` prints, behind those, what fitting the rows' contact forces to the planned motion leaves and changes: one
line per family of the force fit (force_fit.py); CSV and exit status are unchanged.  ``--fit-limits MU,FMAX`` prints the lines of
the fit inside the friction pyramid instead (force_qp.py: friction coefficient MU, force cap FMAX in newtons; ``-`` for either
keeps the planner's); CSV and exit status are unchanged.
"""
import sys

from . import capi, flags
from .planner import LocalPlanner, TOWR_HEIGHTFIELD


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    out, hf, log = "build/traj.csv", None, None
    checked = "--selftest" in argv
    if checked:
        argv.remove("--selftest")
    check = "--check" in argv
    if check:
        argv.remove("--check")
    fit = "--fit" in argv
    if fit:
        argv.remove("--fit")
    limits = None
    for opt in ("--out", "--heightfield", "--log", "--fit-limits"):
        if opt in argv:
            i = argv.index(opt)
            val = argv[i + 1]
            del argv[i:i + 2]
            if opt == "--out":
                out = val
            elif opt == "--log":
                log = val
            elif opt == "--fit-limits":
                mu, f_max = val.split(",")
                limits = {k: float(v) for k, v in (("mu", mu), ("f_max", f_max)) if v != "-"}
                fit = "limits"
            else:
                hf = val
    args = flags.parse_flags(argv)
    lp = LocalPlanner(max_batch=1, checked=checked)
    try:
        import os
        path = hf or TOWR_HEIGHTFIELD
        if os.path.exists(path):
            lp.load_heightfield_file(path, args.get('-resolution'))
        # --log PATH: the per-solve report (report.py) goes to PATH; --log -: to stdout, where it ends with the status line
        # -- the reference's logs/towr_log.out back from `python -m qtos_amd.main ... --log - > logs/towr_log.out`
        try:
            status = lp.solve(args, out_csv=out, log=sys.stdout if log == "-" else log, check=check, fit=fit, limits=limits)
        except capi.SelftestError as e:
            for t in e.attempts:
                print("KKT self-test: " + t.describe())
            print("status -> 2")
            return 2
        if log != "-":
            print("status -> %d" % status)  # the line the reference's log carries (logs/towr_log.out:85)
        return status
    finally:
        lp.close()


if __name__ == "__main__":
    sys.exit(main())
