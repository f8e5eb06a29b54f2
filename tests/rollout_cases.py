"""What the rollout tests share: the plans (as tests/test_plan_check_cpu.py gets them), the gate and the record of the measured
floors (profiles/rollout_accuracy.json is written where QTOS_ROLLOUT_ACCURACY names a file).

The gate for "equals" between the float64 rule (or the kernel) and a longdouble statement is the larger of 8 x the float64-vs-
longdouble floor of the numpy statement measured in the same test and a bound propagated from the roundings, which every test
derives in its docstring; it is capped at CAP = 1e-10 (m, m/s, rad).  u = 2^-53: one rounded operation on v is off by at most
u |v|.

The planner's reference-compat inertia tensor (config.INERTIA_REFERENCE_COMPAT) is the reference's own mix-up of the URDF's six
numbers: it is indefinite, and a PD torque on a body with a negative moment of inertia pushes it away from the plan.  The cases
with gains therefore roll the body out with config.INERTIA_PHYSICAL; the open-loop cases use the planner's own tensor."""
import json
import os

import numpy as np

from conftest import load_gv, oracle_problem

LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
CAP = 1e-10
GAINS = dict(kp_lin=300.0, kd_lin=30.0, kp_ang=30.0, kd_ang=1.0)      # moderate: critically damped translation at 10 rad/s


# The shapes of the kernel test (tests/test_gpu_rollout.py derives them in its docstring), shared with the CPU check that the
# "held" gains and their limit clip some rows and leave few near the limit (tests/test_rollout_cpu.py).
TILE = 256
HZ, N_ROWS = 100.0, 2 * TILE + 37
B = 3
COUNTS = np.array([0, TILE, N_ROWS], np.int32)
T0 = np.array([3.756, 0.0, 11.25])
COUNT_IN = np.array([5, 0, 2], np.int64)
MASS_SCALE = np.array([1.0, 1.0, 1.3])
PUSH = np.zeros((B, 6))
PUSH[2] = (2.0, -1.0, 0.5, 0.02, -0.03, 0.01)
PUSH_FROM, PUSH_TICKS = 302, 40                     # window 2's rows 300 .. 339, window 1's 302 .. 341 (a zero push: the bit alone)
KINDS = {"held": dict(f_fb_max=9.5, **GAINS), "free": dict(ff_scale=0.0)}
NEAR = 1e-9                                         # rows near a limit: within NEAR x limit of it (9.5e-9 N: wider than the 1e-10 gate)


def gate(floor, bound):
    return min(max(8.0 * floor, bound), CAP)


def body_kw(kind, sub, **kw):
    from qtos_amd.config import INERTIA_PHYSICAL
    return dict(inertia_b=INERTIA_PHYSICAL, substeps=sub, push_from=PUSH_FROM, push_ticks=PUSH_TICKS, **KINDS[kind], **kw)


def window_statement(L, cfg, nodes, kind, sub, b, dt, n=None, scale=1.0, joint=None):
    """The statement of window b of the kernel test's base call (`nodes`: the window's plan), with the feedback limits times `scale`."""
    from qtos_amd import rollout as ro
    kw = body_kw(kind, sub)
    if "f_fb_max" in kw:
        kw["f_fb_max"] *= scale
    return ro.rollout_rows(L, nodes, T0[b], HZ, 0, int(COUNTS[b]) if n is None else n, ro.RolloutParams(cfg, **kw), count=int(COUNT_IN[b]),
                           mass_scale=MASS_SCALE[b], push=PUSH[b], joint=joint, dtype=dt)


def near_the_limit(lo, hi):
    """Rows on which bit 3 may differ: where the statements with the limits times 1 - NEAR and 1 + NEAR (their status words `lo`,
    `hi`) disagree on it, a feedback component lies within NEAR of its limit."""
    from qtos_amd import rollout as ro
    return (np.asarray(lo) & ro.CLIPPED) != (np.asarray(hi) & ro.CLIPPED)


def dist(a, b):
    return float(np.abs(np.asarray(a, LD) - np.asarray(b, LD)).max())


def record(name, entry):
    print("rollout accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_ROLLOUT_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


class Plan:
    """A plan of the CPU oracle: the golden walk, a trot, or a step onto the ledges of exp_5 (the base pitches)."""

    def __init__(self, name):
        from oracle import splines as sp
        from oracle.oracle import Oracle, oracle_dict
        from qtos_amd import workloads
        from qtos_amd.config import PlannerConfig
        self.name, height, cell = name, None, 0.1
        gv = load_gv("gv1")
        self.cfg = PlannerConfig.reference_compat(gait="trot") if name == "trot" else PlannerConfig.reference_compat()
        if name == "exp5":
            height, cell = workloads.exp5_terrain()
        self.O = Oracle(oracle_dict(self.cfg), height=height, hcell=cell)
        if name == "walk":
            self.x = np.array(gv["x"])
        elif name == "trot":
            self.x, info = self.O.solve(oracle_problem(self.O, gv["inputs"]))
            assert info.status == 0
        else:
            start, goal = workloads.step_goals(1, seed=1, terrain=(height, cell))
            s = start[0]
            self.x, info = self.O.solve(self.O.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), goal[0]))
            assert info.status == 0
        self.L = sp.layout(self.cfg)
        self.x.setflags(write=False)


_plans = {}


def plan(name):
    if name not in _plans:
        _plans[name] = Plan(name)
    return _plans[name]
