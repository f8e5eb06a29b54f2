#!/usr/bin/env python3
"""Generate tests/golden/towr_log_report.json from the reference's committed solver log (logs/towr_log.out).

Runs only where the reference tree is available; the test-suite uses the committed output.  The fixture holds the log's
dimension block (lines 40-52), its iteration table (lines 54-62) and its final block (lines 64-85) as text, and the values
parsed from them: tests/test_report_format.py feeds the values to qtos_amd.report and compares the text.  Only data of the
log is taken, no source.
"""
import json
import os
import re

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    lines = open(os.path.join(REF, "logs", "towr_log.out")).read().split("\n")
    dims, table, final = lines[39:52], lines[53:62], lines[63:85]
    rows = []
    for ln in table[1:]:
        f = ln.split()
        m = re.match(r"([0-9.e+-]+)([a-zA-Z ]?)$", f[8])
        tag = ln[len(ln) - 4]   # the slot between alpha_pr and the three-wide ls column
        rows.append(dict(iter=int(f[0]), objective=float(f[1]), inf_pr=float(f[2]), inf_du=float(f[3]), lg_mu=float(f[4]),
                         dnorm=float(f[5]), alpha_du=float(f[7]), alpha_pr=float(m.group(1)), tag=tag, ls=int(f[9])))

    def val(prefix):
        ln = next(x for x in final if x.startswith(prefix))
        return ln.split()

    fin = dict(iterations=int(val("Number of Iterations")[-1]),
               inf_du=float(val("Dual infeasibility")[-1]), viol=float(val("Constraint violation")[-1]),
               compl=float(val("Complementarity")[-1]), err=float(val("Overall NLP error")[-1]),
               n_con_evals=int(val("Number of equality constraint evaluations")[-1]),
               n_jac_evals=int(val("Number of equality constraint Jacobian evaluations")[-1]),
               exit=next(x for x in final if x.startswith("EXIT:")), status=int(final[-1].split()[-1]))
    out = dict(source="logs/towr_log.out", dims_lines=dims, table_lines=table, final_lines=final, rows=rows, final=fin)
    with open(os.path.join(OUT, "towr_log_report.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
