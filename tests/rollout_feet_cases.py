"""What the tests of the rollout through the feet share (tests/test_rollout_feet_cpu.py, tests/test_gpu_rollout_feet.py): the
plans (tests/force_fit_cases.py's: the golden walk with three and four stance feet, the trot with two, the flight schedule with
none), the gains, the gates and the recorder (profiles/rollout_feet_accuracy.json is written where QTOS_ROLLOUT_FEET_ACCURACY
names a file).

Gates.  u = 2^-53.  As in tests/rollout_cases.py a gate between the float64 rule (or the kernel) and the longdouble rule is the
larger of 8 x the float64-vs-longdouble floor of the numpy rule measured in the same test and a propagated bound.  The held body's
bounds of tests/test_gpu_rollout.py (POS = 256 u on r and q, RATE = 2^15 u on v, w_b and R w_b, EULER = 2^12 u, 4 POS on |e| and
the tilt) are taken over for the state, with one change: the feedback wrench now goes through a 6 x 6 solve.  Its right-hand side
rho~ = (tau_fb / arm, F_fb) differs between two evaluations by e~ = (kp_ang 2 POS + kd_ang RATE) / arm + kp_lin POS + kd_lin RATE
= (30 x 512 u + 2^15 u) / 0.2 + 300 x 256 u + 30 x 2^15 u < 2^21 u newtons, and the solve amplifies a relative perturbation by K,
the largest 2-norm condition number of M on the rows compared (measured in float64 with numpy.linalg.cond and recorded): on rows
with two stance feet K is of the order of W / (damping n) = 1e6, and what the amplification acts on is only the part of the wrench
the two feet cannot deliver, which the damping keeps out of the forces: df = w A~^T y with |y| <= |rho~| / lambda_min in that one
direction and A~^T y = 0 along it but for the damping.  The bound used is therefore the one of tests/force_fit_cases.py, K e~ on
the forces and 4 K e~ on the three norms, and the state's bound grows by h / m_s (and h |l| / I_min for the rotation) times the
force's per step of the loop's memory -- which the held loop forgets within about 1 / (h kd / I) steps; with h <= 0.01 s, m_s >=
3 kg, |l| <= 0.5 m, I_min = 0.0058 kg m^2 the factor is below 1 per step, so the state's bound is the larger of the held body's
and K e~ x 2^-10.  Every gate is the larger of its bound and 8 x the measured floor; there is no fixed cap (force_fit_cases' rule)."""
import json
import os

import numpy as np

import force_fit_cases as ffc
import rollout_cases as rc

LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
GAINS = rc.GAINS
E_RHS = 2.0 ** 21 * U                       # e~ of the docstring [N]
POS, RATE, EULER = 256 * U, 2 ** 15 * U, 2 ** 12 * U
ROW_GROUPS = dict(r=(slice(1, 4), POS), euler=(slice(4, 7), EULER), v=(slice(7, 10), RATE), Rw=(slice(10, 13), RATE), q=(slice(13, 17), POS),
                  norms=(slice(17, 19), 4 * POS), fb=(slice(19, 20), E_RHS))
FEET_GROUPS = dict(f_a=(slice(1, 13), 1.0), missing=(slice(13, 15), 4.0), change=(slice(15, 16), 4.0))

plan = ffc.plan
dist = ffc.dist
condition = ffc.condition


def state_gate(floor, bound, K):
    return max(8.0 * float(floor), bound, K * E_RHS * 2.0 ** -10)


def feet_gate(floor, factor, K):
    return max(8.0 * float(floor), factor * K * E_RHS)


def same(a, b):
    """Equal to the bit (a longdouble's padding bytes are not part of it; NaNs in the same places)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype == F64:
        return a.shape == b.shape and a.tobytes() == np.asarray(b, F64).tobytes()
    return np.array_equal(a, b, equal_nan=True) and np.array_equal(np.signbit(a), np.signbit(b))


def record(name, entry):
    print("rollout feet accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_ROLLOUT_FEET_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
