#!/usr/bin/env python3
"""The clip-against-QP table of DESIGN.md section 6 ("Rollout with the force QP"), in float64 numpy (no GPU): the closed loop of
tests/rollout_cases.py's windows with rollout_feet.py's clip (FEET_LIMIT) and with rollout_qp.py's QP at the same limits -- the
largest undelivered force and moment over the alive rows, the largest tilt, the first frozen row.  scratch/rollout_qp_table.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import force_fit_cases as ffc  # noqa: E402
import rollout_cases as rc  # noqa: E402
import rollout_qp_cases as qc  # noqa: E402
from qtos_amd import rollout as ro, rollout_feet as rf, rollout_qp as rq  # noqa: E402

CASES = (("walk", 1, 100.0, 0.7, 14.0), ("walk", 2, 100.0, 0.7, 14.0), ("trot", 1, 100.0, 0.3, 20.0))
for name, b, hz, mu, f_max in CASES:
    P = ffc.plan(name)
    n = int(rc.COUNTS[1])
    rp = ro.RolloutParams(P.cfg, **qc.body_kw(1))
    kw = dict(count=int(rc.COUNT_IN[b]), mass_scale=rc.MASS_SCALE[b], push=rc.PUSH[b], dtype=np.float64)
    clip = rf.rollout_feet_rows(P.L, P.x, rc.T0[b], hz, 0, n, rp, rf.FeetParams(P.cfg, mu=mu, f_max=f_max, damping=1e-2, limit=True), **kw)
    qp = rq.rollout_qp_rows(P.L, P.x, rc.T0[b], hz, 0, n, rp, rq.QpFeetParams(P.cfg, mu=mu, f_max=f_max, damping=1e-2), detail=True, stop_tests=False, **kw)
    for what, rows, frows, status, steps in (("clip", clip[1], clip[2], clip[3], None), ("qp", qp[1], qp[2], qp[4], qp[8]["steps"])):
        alive = (status & 3) == 0
        frozen = int(np.argmax(~alive)) if not alive.all() else -1
        line = "%-4s window %d mu %.1f f_max %4.1f %-4s miss_f %6.2f N  miss_t %5.2f N m  tilt %.3f rad  frozen at %4d  limited %3d" % (
            name, b, mu, f_max, what, frows[alive, 13].max(), frows[alive, 14].max(), rows[alive, 18].max(), frozen, int(((status & 256) != 0).sum()))
        if steps is not None:
            line += "  most steps %d  cap %d" % (int(steps.max()), int(((status & 512) != 0).sum()))
        print(line, flush=True)
