"""What the plan-check tests share (tests/test_plan_check_cpu.py, tests/test_gpu_plan_check.py): the oracle's time grids as it
forms them, the propagated error bounds of the column groups, and the recorder of what the tests measure.

Error bounds.  u = 2^-53; one rounding of v is at most u |v|.  The plans of the tests stay within: base positions and feet
1 m, Euler angles 0.5 rad, base velocity 1 m/s, foot velocity 2 m/s, jerk of the base 500 m/s^3 and 100 rad/s^3, foot forces
30 N with slopes up to 1000 N/s, lever arms |r - p_e| 0.5 m, T = 5 s in at most 52 polynomials per spline.  Two evaluations of
one row differ in

  local time  each forms the start of a polynomial from a running sum of up to 52 durations, every rounding at most 5 u s:
              500 u s between the two (the longdouble statement has no such term: it is the floor's as well)
  positions   four Hermite weights <= 1 of six operations, values <= 1 m: 10 u m, and 2 m/s x 500 u s: 1010 u m
  rom         R^T (p - r): both positions (2020 u m) and nine entries of R at 4 u each (sines and cosines at 1 u in numpy and
              the C library; the device's at an ASSUMED 4 ulp: 16 u per entry) over 0.5 m:               2100 u m  (2.4e-13 m)
  terrain     z of a foot and the table's height, no arithmetic but one subtraction; a foot's z moves at 2 m/s:  1010 u m  (1.2e-13 m)
  force       a force of 30 N through weights <= 1: 300 u N, and 1000 N/s x 500 u s = 5e5 u N;
              the basis of a slope of at most 3 adds 40 u relative:                                     5.1e5 u N  (5.7e-11 N)
  dyn_lin     m a with weights of 6 / T^2 = 600 on positions of 1 m (4000 u m/s^2) and 500 m/s^3 x 500 u s:     7.6e5 u N  (8.5e-11 N)
  dyn_ang     four lever-arm products of forces off by 5.1e5 u N over 0.5 m:                                1.0e6 u N m (1.1e-10 N m)

The local-time term dominates all but the first three and is a worst case over 52 roundings of one sign.  Every gate is
the larger of this bound and 8 x the float64 statement's measured distance from its longdouble form, capped at 1e-10, so
dyn_ang is held by the cap.  The device evaluates the float64 statement's formulas with fused multiply-adds and its own
sincos (ASSUMED 4 ulp): the same bounds with the 16 u per entry of R already counted above.
"""
import json
import os

import numpy as np

U = 2.0 ** -53
CAP = 1e-10
BOUND = {"dyn_ang": 1.0e6 * U, "dyn_lin": 7.6e5 * U, "rom": 2100 * U, "terrain": 1010 * U, "force": 5.1e5 * U}
GROUPS = {"dyn_ang": slice(1, 4), "dyn_lin": slice(4, 7), "rom": slice(7, 19), "terrain": slice(19, 23), "force": slice(23, 27)}
TOL = (1e-3, 1e-2, 1e-4, 1e-4, 1e-2)


def gate(group, floor):
    """The gate of a column group: the larger of 8 x the measured float64 floor and the propagated bound, capped."""
    return min(CAP, max(8.0 * float(floor), BOUND[group]))


def oracle_times(T, dt):
    """The oracle's time grid as time_grid forms it: t += dt accumulated over floor(T / dt) steps, then T."""
    assert dt >= T / 520, "the oracle's time arrays hold 524 entries and are not checked"
    out, t = [0.0], 0.0
    for _ in range(int(np.floor(T / dt))):
        t += dt
        out.append(t)
    out.append(T)
    return np.array(out)


def node_times(S):
    """The times of a spline's nodes as the oracle's locate meets them: the durations summed one by one."""
    return np.concatenate([[0.0], np.cumsum(np.asarray(S.dur, np.float64))])


def record(name, entry):
    print("plan check accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_PLAN_CHECK_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
