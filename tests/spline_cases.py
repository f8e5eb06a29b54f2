"""Shared by test_splines_cpu.py and test_gpu_splines.py: the transcriptions the spline layer is checked on, seeded
problems and random plans, the variable / column groups of the accuracy gates.  No tests in here."""
import json
import os

import numpy as np

from conftest import ROOT  # noqa: F401  (path set-up)

from oracle import splines as sp
from oracle.oracle import Oracle, oracle_dict
from qtos_amd.config import PlannerConfig

TRANSCRIPTIONS = {
    "walk": lambda: PlannerConfig.reference_compat(),
    "trot": lambda: PlannerConfig.reference_compat(gait="trot"),
    "knots100_trot": lambda: PlannerConfig.knots100(gait="trot"),
    "knots200_vel": lambda: PlannerConfig.knots200(honor_start_velocity=True),
    "short_last_poly": lambda: PlannerConfig(duration=2.5, dt_base=0.2, dt_dynamic=0.2),      # 12 x 0.2 s + 0.1 s
    "two_base_polys": lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5),
}
NAMES = list(TRANSCRIPTIONS)

GROUPS = ("motion_values", "motion_velocities", "force_values", "force_derivatives")
GATE_FACTOR, GATE_CAP = 8.0, 1e-10
NOISE_MOTION, NOISE_FORCE = 0.1, 20.0

_cache = {}


def case(name):
    """(cfg, Oracle on flat ground, layout) of a transcription, built once."""
    if name not in _cache:
        cfg = TRANSCRIPTIONS[name]()
        _cache[name] = (cfg, Oracle(oracle_dict(cfg)), sp.layout(cfg))
    return _cache[name]


def var_groups(L):
    """Group (index into GROUPS) of every variable."""
    return 2 * (L.var_set >= 6) + L.var_is_vel


def row_groups():
    """Group of every CSV column but the time stamp (column 0: -1)."""
    g = np.zeros(37, int)
    g[0] = -1
    g[19:25] = 1
    g[25:37] = 2
    return g


def problems(n, seed):
    """Seeded starts [n, 24] and goals [n, 3]: a shifted CoM, a small attitude, feet off their nominal places, non-zero
    start velocities (start[18:24])."""
    from qtos_amd import workloads
    rng = np.random.default_rng(seed)
    start = np.stack([workloads.rest_start(x, y, z) for x, y, z in
                      zip(rng.uniform(0.0, 2.0, n), rng.uniform(-0.3, 0.3, n), rng.uniform(0.22, 0.27, n))])
    start[:, 3:6] += rng.normal(0.0, 0.05, (n, 3))
    start[:, 6:18] += rng.normal(0.0, 0.02, (n, 12))
    start[:, 18:24] = rng.normal(0.0, 0.2, (n, 6))
    goal = np.stack([start[:, 0] + rng.uniform(0.3, 0.6, n), start[:, 1] + rng.uniform(-0.05, 0.05, n), np.full(n, 0.24)], axis=1)
    return start, goal


def oracle_problem(O, cfg, s, g):
    """The oracle's problem of a start vector and goal: the start velocities only where the configuration honours them
    (a configuration that does not starts from rest whatever start[18:24] says)."""
    hv = bool(cfg.honor_start_velocity)
    return O.problem(s[0:3], s[3:6], s[6:18].reshape(4, 3), g, s[18:21] if hv else (0, 0, 0), s[21:24] if hv else (0, 0, 0))


def random_plans(name, n, seed):
    """n random plans of a transcription: the straight-line guess of a seeded problem plus seeded noise (sigma 0.1 on motion
    variables, 20 on force variables).  The kernels are linear in the nodes: no solve is needed, and with random nodes an
    index error is an error of order 0.1 (20 N).  Returns (plans [n, n_vars], start, goal)."""
    cfg, O, L = case(name)
    start, goal = problems(n, seed)
    rng = np.random.default_rng(seed + 1000)
    sigma = np.where(L.var_set >= 6, NOISE_FORCE, NOISE_MOTION)
    x = np.stack([O.initial_guess(oracle_problem(O, cfg, start[b], goal[b])) for b in range(n)])
    return x + rng.normal(size=x.shape) * sigma, start, goal


def group_max(err, groups):
    """Largest |err| per group: err [..., n] against groups [n] (-1: not in any group)."""
    err = np.abs(np.asarray(err, np.longdouble)).reshape(-1, len(groups))
    return {GROUPS[k]: float(err[:, groups == k].max()) for k in range(len(GROUPS)) if (groups == k).any()}


def gates(floor):
    """The gate of every group: its rounding floor times 8, never above 1e-10."""
    return {k: min(GATE_FACTOR * v, GATE_CAP) for k, v in floor.items()}


def merge_max(a, b):
    return {k: max(a.get(k, 0.0), b.get(k, 0.0)) for k in set(a) | set(b)}


def record(section, name, floor, achieved):
    """Print a check's rounding floor and achieved error per group; where the environment variable QTOS_SPLINE_ACCURACY
    names a file, keep them in it as JSON (profiles/spline_accuracy.json is such a file from an MI355X run)."""
    entry = dict(floor=floor, gate=gates(floor), gpu_error=achieved)
    print("spline accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_SPLINE_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def assert_within(achieved, floor, what):
    g = gates(floor)
    for k, v in achieved.items():
        assert v <= g[k], "%s, %s: error %.3e above the gate %.3e (floor %.3e)" % (what, k, v, g[k], floor[k])
