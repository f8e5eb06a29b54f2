"""Shared by test_step_cpu.py and test_gpu_steps.py: the solves on which every interior-point step of k_start / k_step
(csrc/kernels.hpp) is held to the restatement oracle/ipm.py -- the smallest transcription on each path of k_step's row code --,
their inputs, the restatement's own run of each (cached), the gates, the accuracy record.  No tests in here.

k_step keeps a thread's first KR = 2 inequality rows and KE = 2 equality rows in registers (ET = 512 threads: 1024 rows of
either kind) and sends the rest through memory; the cases sit on either side of those limits
(test_the_case_table_sits_on_the_paths_it_names holds them to the figures below).
"""
import dataclasses
import json
import os

import numpy as np

from conftest import ROOT, load_gv, start_vector  # noqa: F401  (path set-up)

import linearisation_cases as lc
import spline_cases as sc
from oracle import ipm
from oracle.oracle import Oracle, oracle_dict
from qtos_amd import workloads
from qtos_amd.config import PlannerConfig

ET, KR, KE = 512, 2, 2                     # csrc/kernels.hpp
GATE_VALUE, GATE_ENTRY = lc.GATE_VALUE, lc.GATE_ENTRY
GATE_DIRECTION = 5e-6                      # the KKT gate in the header of test_gpu_parity.py, of the step's largest entry
GATE_NODES = 1e-6                          # the project's full-solve gate (restatement against the C oracle)
U = 2.0 ** -53                             # unit roundoff of float64


def _flat(n, seed, pick=None):
    def f(cfg):
        start, goal = workloads.flat_goals(128 if pick else n, seed=seed)
        idx = list(pick) if pick else list(range(n))
        return start[idx], goal[idx], None, None
    return f


def _steps(n, seed, mode):
    def f(cfg):
        t = workloads.exp5_terrain()
        start, goal = workloads.step_goals(8, seed=seed, terrain=t, mode=mode)
        return start[:n], goal[:n], t, None
    return f


def _first_of_seeds(seeds, mode):
    """Problem 0 of step_goals(8, seed) for every seed."""
    return _picked([(s, 0) for s in seeds], mode)


def _picked(pairs, mode):
    """Problem b of step_goals(8, seed) for every (seed, b)."""
    def f(cfg):
        t = workloads.exp5_terrain()
        sg = [workloads.step_goals(8, seed=s, terrain=t, mode=mode) for s, _ in pairs]
        return (np.stack([sg[i][0][b] for i, (_, b) in enumerate(pairs)]), np.stack([sg[i][1][b] for i, (_, b) in enumerate(pairs)]),
                t, None)
    return f


def _gv1(cfg):
    gv = load_gv("gv1")
    return start_vector(gv["inputs"])[None], np.array(gv["inputs"]["g"], float)[None], None, gv["x"][None]


# name: (configuration, inputs, steps, the reduced system too, inequality rows, what the case is there for)
CASES = {
    # 208 threads without a row, no second register row
    "two_base_polys": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5), _flat(4, 3), 8, False, 304,
                       "fewer rows than threads"),
    # the second register row half valid (652 - 512 = 140 threads have one)
    "short_last_poly": (lambda: PlannerConfig(duration=2.5, dt_base=0.2, dt_dynamic=0.2), _flat(4, 3), 8, False, 652,
                        "second register row half valid"),
    # exactly the register limit; the logged cold start: amax 0.68 - 0.75 and az 0.25 in the first step
    "walk": (lambda: PlannerConfig.reference_compat(), _flat(4, 3), 8, True, 1024, "all rows in registers, none beyond"),
    # 132 inequality rows go through memory (dzl / dzu stored in the ratio pass, re-read in the update pass).  None of the first
    # 24 goals of flat_goals(128, seed=0) takes two chord steps in a row on this transcription (searched on the CPU): the two
    # chord steps in a row are in knots100_trot
    "trot": (lambda: PlannerConfig.reference_compat(gait="trot"), _flat(4, 0, pick=(1, 2, 3, 4)), 8, True, 1156, "inequality tail through memory"),
    # more than 1024 equality rows: the equality tail goes through memory, with the gt -> g copy; the goals of
    # test_second_chord_step_finishes_the_trot_batch (plain mu rule) that take two chord steps in a row
    "knots100_trot": (lambda: PlannerConfig.knots100(gait="trot", mu_superlinear=False), _flat(2, 0, pick=(4, 5)), 6, True, 1156,
                      "equality tail through memory, two chord steps in a row"),
    # 2080 inequality rows: a tail three rows deep (four steps of the six the solves take: every step runs the tail, and a
    # dense solve of its 3390 unknowns is what the test's time goes into)
    "walk12": (lambda: PlannerConfig.reference_compat(duration=12.0), _flat(2, 3), 4, False, 2080, "a three-deep inequality tail"),
    # bilinear exp_5 ramps on the smallest transcription: line searches of 2 to 6 trials (problems picked from 24 searched on
    # the CPU: those with more than one trial on which qo_solve can be the CPU test's reference, see bilinear_steps)
    "bilinear_1s": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5, terrain_mode=0),
                    _picked(((1, 0), (2, 2), (3, 3), (5, 1)), 0), 6, False, 304, "line searches with more than one trial, smallest transcription"),
    # the same ramps on the 2.5 s transcription, kept next to the 1 s one for what that one does not show: steps whose six trials
    # all fail, and (seed 1) a solve that stalls under the product's settings -- test_step_cpu.py and test_gpu_steps.py run it
    # with the stall rules on as well.  Seeds and steps: those on which qo_solve can be the CPU test's reference.  qo_solve takes
    # the Jacobian's pattern from ONE evaluation at a perturbed starting point and reads the Jacobian through that pattern only;
    # on the bilinear map a terrain slope that is zero there (a flat cell) and 2.75 or 4.4 at a later iterate is left out of its
    # KKT system (seed 0: 11 entries at the starting point already), and its steps part from the restatement's, which uses the
    # whole Jacobian -- on most seeds within two steps, on seeds 1 and 3 behind the fifth, on seed 13 not at all
    "bilinear_steps": (lambda: PlannerConfig(duration=2.5, dt_base=0.2, dt_dynamic=0.2, terrain_mode=0), _first_of_seeds((13, 1, 3), 0), 5,
                       False, 652, "line searches with more than one trial, six failing trials, a stalled solve"),
    # two of the seeds on which qo_solve parts from the restatement (seed 0 in the first step, seed 4 in the second): the GPU
    # test needs the oracle's constraints and Jacobian only, and holds the kernels to the restatement there; no qo_solve test
    "bilinear_no_qo": (lambda: PlannerConfig(duration=2.5, dt_base=0.2, dt_dynamic=0.2, terrain_mode=0), _first_of_seeds((0, 4), 0), 5,
                       False, 652, "steps on which qo_solve leaves slopes out of its system"),
    # nearest-cell exp_5, the default settings: the hold latches
    "hold": (lambda: PlannerConfig.reference_compat(), _steps(4, 3, 1), 8, False, 1024, "the hold latch on a terrain"),
    # the gv1 warm start: warm_slack_push
    "warm": (lambda: PlannerConfig.reference_compat(), _gv1, 8, False, 1024, "a warm start"),
    # the settings of PlannerConfig.receding_windows on the reference transcription
    "plain_mu": (lambda: PlannerConfig.reference_compat(mu_superlinear=False, chord_tol=0.0), _flat(4, 3), 8, False, 1024,
                 "the plain mu rule, no chord steps"),
}
NAMES = list(CASES)
QO_NAMES = [n for n in NAMES if n != "bilinear_no_qo"]      # the cases on which qo_solve is a reference
STALLED = ("bilinear_steps", 1)                               # (case, problem) that stalls under the product's settings
REDUCED_NAMES = [n for n in NAMES if CASES[n][3]]
# Searched on the CPU and not found (oracle/ipm.py's events; 24 trot goals under either mu rule, 12 seeds each of step_goals on
# the bilinear and nearest-cell exp_5 map, both transcriptions, 10 goals of the 100-knot trot, 138 further nearest-cell exp_5
# solves on the 2.5 s and the reference transcription): a solve whose chord step is discarded, and a step on which the clip of
# z is active.  No case has either.  Of the 56 bilinear solves searched under the product's stall settings four stall and none
# jams (two steps in a row shorter than stall_alpha): the jam rule's stop is not covered.
NOT_FOUND = ("a discarded chord step", "an active clip of z", "a jammed solve")

_cache, _runs = {}, {}


class Case:
    pass


def prefix(cfg):
    """The prefix planners run without the stall rules: a stalled or jammed solve hands back its best iterate, not its last."""
    return dataclasses.replace(cfg, stall_iters=0, stall_alpha=0.0)


def case(name):
    if name not in _cache:
        make, inputs, steps, reduced, n_iq, why = CASES[name]
        c = Case()
        c.name, c.steps, c.reduced, c.n_iq, c.why = name, steps, reduced, n_iq, why
        c.product_cfg = make()
        c.cfg = prefix(c.product_cfg)                   # the reduced system on, as the table has it
        c.cfg_full = lc.full(c.cfg)
        c.product_full = lc.full(c.product_cfg)        # the full system with the product's stall rules and max_iter
        c.start, c.goal, c.terrain, c.warm = inputs(c.cfg)
        kw = dict(height=c.terrain[0], hcell=c.terrain[1]) if c.terrain else {}
        c.O = Oracle(oracle_dict(c.cfg_full), **kw)     # (full system: the starting point is towr's guess as it is)
        c.B = len(c.start)
        c.q = [sc.oracle_problem(c.O, c.cfg, c.start[b], c.goal[b]) for b in range(c.B)]
        _cache[name] = c
    return _cache[name]


def run(name, b, cfg=None):
    """The restatement's own run of problem b of a case (full system, stall rules off unless cfg says otherwise), cached."""
    key = (name, b, None if cfg is None else (cfg.stall_iters, cfg.stall_alpha))
    if key not in _runs:
        c = case(name)
        _runs[key] = ipm.solve(c.O, c.q[b], cfg or c.cfg_full, x0=None if c.warm is None else c.warm[b], max_iter=c.steps)
    return _runs[key]


def exclusion_margin(n_rows):
    """An Armijo decision closer than this to its right-hand side is not decided by the test: the l1 sum's own uncertainty,
    the number of working rows times the gate on a constraint value."""
    return n_rows * GATE_VALUE


def armijo_decision(th, rhs, margin):
    """A trial's acceptance -- th <= rhs or th < 1e-9 -- when th is only known to within `margin`: True, False, or None where
    the decision depends on which way the uncertainty falls (a robustly met Armijo test decides whatever the floor test says)."""
    a = True if th <= rhs - margin else (False if th > rhs + margin else None)
    b = True if th < ipm.TH_FLOOR - margin else (False if th >= ipm.TH_FLOOR + margin else None)
    if a is True or b is True:
        return True
    return False if (a is False and b is False) else None


def record(section, name, entry):
    """Print a check's figures; where the environment variable QTOS_STEP_ACCURACY names a file, keep them in it as JSON
    (profiles/step_accuracy.json is such a file)."""
    print("step accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_STEP_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
