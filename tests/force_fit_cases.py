"""What the force-fit tests share (tests/test_force_fit_cpu.py, tests/test_gpu_force_fit.py): the plans, the gates of the column
groups with their derivation, the comparison per stance count, and the recorder of what the tests measure.

Plans.  Plan("walk" | "trot" | "exp5") are the three plans of tests/test_plan_check_cpu.py, built the same way: the golden walk,
the reference_compat trot solved by the oracle, a walk onto the ledges of exp_5.  Their rows have 2, 3 or 4 stance feet, never
none, so Plan("flight") adds rows without a stance foot: a 1 s schedule in which every foot stands 0.3 s, flies 0.2 s and stands
0.5 s, under the oracle's straight-line guess with a smooth perturbation of every node -- not a solved plan, and it need not be
one: the fit reads the nodes as data.

Gates.  u = 2^-53.  tests/plan_check_cases.py bounds what two evaluations of one row differ in: the dynamics rows by
e_lin = BOUND["dyn_lin"] = 7.6e5 u N and e_ang = BOUND["dyn_ang"] = 1.0e6 u N m.  The fit solves M y = rho~ with rho~ = (rho_ang /
arm, rho_lin), so its right-hand side differs by e~ = e_ang / arm + e_lin newtons, and a solve with the matrix M amplifies a
relative perturbation of its data by cond(M): with K the largest 2-norm condition number of M over the rows compared (measured
in float64 with numpy.linalg.cond, and stated with every comparison),

  f_fit    columns  1 .. 12   df_e = w_e A~_e^T y, |A~_e^T| of the order of 1 (lever arms of at most 2.5 arms):        K e~
  res_ang  columns 13 .. 15   rho_ang - sum (p_e - r) x df_e: its own e_ang and four lever arms of 0.5 m:            e_ang + 2 K e~
  res_lin  columns 16 .. 18   rho_lin - sum df_e:                                                                    e_lin + 4 K e~
  change   column  19         the 2-norm of twelve components:                                                       4 K e~
  tau      columns 20 .. 31   -J^T R^T f_fit: the rows of J^T sum to less than 1 m (links of 0.16 m, a lateral offset of 0.06 m),
                              R's entries at 16 u over 30 N:                                                         K e~ + 500 u

K is of the order of 1 / damping on rows with two stance feet (the support cannot carry the moment about the line through the
feet: W / (damping n) = 2 / 2e-6; measured 4e6 .. 5.4e6 on the plans here), 1e3 .. 2e3 on rows with three and 20 .. 1.2e3 on rows
with four (the load weights reach down to w_min = 0.01).  So rows are compared per stance count, each count with its own K.
Every gate is the larger of this bound and 8 x the float64 statement's measured distance from its longdouble form on the same
rows.  There is no fixed cap: what limits a gate is that factor of 8 over the float64 floor.  Rows without a stance foot have
nothing solved (K = 1), and their f_fit is the plan's force to the bit, which the tests assert apart.
"""
import json
import os

import numpy as np

import plan_check_cases as pcc
from conftest import load_gv, oracle_problem

U = pcc.U
LD, F64 = np.longdouble, np.float64
GROUPS = {"f_fit": slice(1, 13), "res_ang": slice(13, 16), "res_lin": slice(16, 19), "change": slice(19, 20), "tau": slice(20, 32)}
TOL = (1e-3, 1e-2, 5.0, 1e-2)


def bound(group, cond, arm=0.2):
    """The propagated bound of a column group on rows whose M has a condition number of at most cond (the derivation above)."""
    e_lin, e_ang = pcc.BOUND["dyn_lin"], pcc.BOUND["dyn_ang"]
    k = float(cond) * (e_ang / float(arm) + e_lin)
    return {"f_fit": k, "res_ang": e_ang + 2 * k, "res_lin": e_lin + 4 * k, "change": 4 * k, "tau": k + 500 * U}[group]


def gate(group, floor, cond, arm=0.2):
    """The gate of a column group: the larger of 8 x the measured float64 floor and the propagated bound."""
    return max(8.0 * float(floor), bound(group, cond, arm))


def condition(M, rows):
    """The largest 2-norm condition number of M [n, 6, 6] over the rows `rows` (a mask); 1 where nothing is solved."""
    M = np.asarray(M, F64)[rows]
    if not len(M) or not np.abs(M).max() > 0:
        return 1.0
    return float(np.linalg.cond(M).max())


def dist(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.abs(a - b).max()) if a.size else 0.0


def compare(got, want_ld, want_64, detail_64, arm=0.2, groups=GROUPS, rows=None):
    """`got` [n, 32] against the longdouble statement per stance count and column group: {count: {group: dict(err, floor, gate,
    cond, rows)}}, floor the float64 statement's distance from the longdouble one on the same rows."""
    cnt = detail_64["stance"].sum(axis=1)
    out = {}
    for c in sorted(set(int(v) for v in cnt)):
        m = cnt == c
        if rows is not None:
            m = m & rows
        if not m.any():
            continue
        K = condition(detail_64["M"], m) if c else 1.0
        out[c] = {}
        for group, cols in groups.items():
            floor, err = dist(want_64[m][:, cols], want_ld[m][:, cols]), dist(np.asarray(got)[m][:, cols], want_ld[m][:, cols])
            out[c][group] = dict(err=err, floor=floor, gate=gate(group, floor, K, arm), cond=K, rows=int(m.sum()))
    return out


def assert_within(cmp, what=""):
    for c, groups in cmp.items():
        for group, w in groups.items():
            assert w["err"] <= w["gate"], (what, "stance feet", c, group, w)


class Plan:
    """One of the plans above: cfg, the spline layout L, the nodes x, the terrain (None: flat ground)."""

    def __init__(self, name):
        from oracle import splines as sp
        from oracle.oracle import Oracle, oracle_dict
        from qtos_amd import workloads
        from qtos_amd.config import PlannerConfig
        self.name, self.terrain, height, cell = name, None, None, 0.1
        if name == "flight":
            self.cfg = PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5,
                                     phase_durations=[[0.3, 0.2, 0.5]] * 4)
        else:
            self.cfg = PlannerConfig.reference_compat(gait="trot") if name == "trot" else PlannerConfig.reference_compat()
        if name == "exp5":
            height, cell = workloads.exp5_terrain()
            self.terrain = (height, cell, -1.0, -1.0)
        self.O = Oracle(oracle_dict(self.cfg), height=height, hcell=cell)
        if name == "walk":
            self.x = np.array(load_gv("gv1")["x"])
        elif name == "trot":
            self.x, info = self.O.solve(oracle_problem(self.O, load_gv("gv1")["inputs"]))
            assert info.status == 0
        elif name == "exp5":
            start, goal = workloads.step_goals(1, seed=1, terrain=(height, cell))
            s = start[0]
            self.x, info = self.O.solve(self.O.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), goal[0]))
            assert info.status == 0
        else:
            self.x = flight_nodes(self.O)
        self.L = sp.layout(self.cfg)
        self.x.setflags(write=False)


def flight_nodes(O):
    """Nodes for the flight schedule: the oracle's straight-line guess from rest to 9 cm ahead, every node moved by a smooth 2 %
    (1 mm .. 1 cm, a few tenths of a newton)."""
    from qtos_amd import workloads
    s = workloads.rest_start(0.1)
    x = np.array(O.initial_guess(O.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), np.array([0.19, 0.0, 0.24]))), F64)
    i = np.arange(len(x), dtype=F64)
    return x + 0.02 * np.sin(0.37 * i + 0.5) * np.maximum(np.abs(x), 0.05)


_plans = {}


def plan(name):
    if name not in _plans:
        _plans[name] = Plan(name)
    return _plans[name]


def record(name, entry):
    print("force fit accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_FORCE_FIT_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
