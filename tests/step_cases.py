"""Shared by test_step_cpu.py and test_gpu_steps.py: the solves on which every interior-point step of k_start / k_step
(csrc/kernels.hpp) is held to the restatement oracle/ipm.py -- the smallest transcription on each path of k_step's row code --,
their inputs, the restatement's own run of each (cached), the gates, the accuracy record.  No tests in here.

k_step keeps a thread's first KR = 2 inequality rows and KE = 2 equality rows in registers (ET = 512 threads: 1024 rows of
either kind) and sends the rest through memory; the cases sit on either side of those limits
(test_the_case_table_sits_on_the_paths_it_names holds them to the figures below).  Three paths the product's settings do not
take -- a discarded chord step, an active clip of z, the jam stop -- have cases and STOPPED entries under settings that reach them.
"""
import dataclasses
import json
import os

import numpy as np

from conftest import ROOT, load_gv, start_vector  # noqa: F401  (path set-up)

import linearisation_cases as lc
import spline_cases as sc
from oracle import duals, ipm
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


def _far(pairs, mode, dx):
    """_picked with every goal moved dx metres in x: out of the plan's reach."""
    def f(cfg):
        start, goal, t, _ = _picked(pairs, mode)(cfg)
        goal = goal.copy()
        goal[:, 0] += dx
        return start, goal, t, None
    return f


WIDE = 2.5                                  # `groups`: the nominal stance's x and y scaled by this


def _wide_stance():
    return tuple((WIDE * x, WIDE * y, z) for x, y, z in PlannerConfig().nominal_stance)


def _groups(cfg):
    """Three warm starts, one per group of unknowns that attains the dual infeasibility in no other case (searched on the CPU,
    test_duals_cpu.py holds the outcome): a robot standing still -- the goal 2 cm from the start, the feet on the nominal stance,
    so that towr's straight-line guess leaves every range-of-motion row its whole band and z_u - z_l all but cancels -- with ONE
    node moved far enough to violate a few rows, whose z = mu / warm_slack_push then stand alone.  Problem 0: the yaw of base
    node 8 by 0.2 rad -- both horizontal range-of-motion rows of all four feet at t = 0.8 s, with levers of 0.425 and 0.5 m (the
    stance 2.5 times as wide as the default: with its levers of 0.17 and 0.2 m a foothold, whose entries are 1, wins); problem
    1: the height of base node 12 by 0.1 m -- the vertical rows of all four feet; problem 2: the normal force of one stance
    node of foot 0 to -50 N -- its unilateral row and its four friction rows.  The nodes are put into the reduced system's space
    (the base spline projected, the swings on their rule), so that both systems start from the same point."""
    from oracle import projection
    start, goal = workloads.flat_goals(4, seed=3)
    start, goal = np.repeat(start[:1], 3, axis=0), np.repeat(goal[:1], 3, axis=0)
    for e in range(4):
        start[:, 6 + 3 * e:8 + 3 * e] = start[:, :2] + np.array(cfg.nominal_stance[e][:2])
    goal[:] = start[:, :3] + np.array([0.02, 0.01, 0.0])
    O = Oracle(oracle_dict(lc.full(cfg)))
    warm = []
    for b in range(3):
        q = sc.oracle_problem(O, cfg, start[b], goal[b])
        xl, xh = O.var_bounds(q)
        x = O.initial_guess(q)
        v, dv = ((O.L.off_ang + 6 * 8 + 2, 0.2), (O.L.off_lin + 6 * 12 + 2, 0.1), (O.L.off_eef[0] + 52, -50.0))[b]
        assert xl[v] != xh[v]
        x[v] += dv
        warm.append(O.project_swings(projection.project_nodes(x, O.L, (xl != xh).astype(np.int32))))
    return start, goal, None, np.stack(warm)


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
    # ---- the paths the product's settings do not take (searched, see NOT_FOUND): settings that put the smallest transcriptions
    # on them.  chord_tol = 1e3 sends a chord step behind the FIRST full step, at a violation of 1 to 10, where the old
    # factorisation is no use: its line search ends below 1 and the step is discarded (kinds 0, 2, 0, 0) ----
    "discard_small": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5, chord_tol=1e3, chord_shrink=1.0),
                      _flat(4, 3), 4, True, 304, "a discarded chord step (two trials), the fresh step behind it"),
    # bilinear_1s' problems 1 and 2: the discarded step ends a search of 3 and 4 trials, the fresh step behind it is damped
    # (alpha 0.25, three trials)
    "discard_bilinear": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5, terrain_mode=0,
                                               chord_tol=1e3, chord_shrink=1.0),
                         _picked(((2, 2), (3, 3)), 0), 6, False, 304, "a chord step discarded behind a search of several trials, a damped step behind it"),
    # kappa_sigma = 10: z x gap leaves [mu / 10, 10 mu] on the first two steps (alpha = 1: mu moves, so the clip at the new mu
    # would be another)
    "clip_small": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5, kappa_sigma=10.0), _flat(4, 3), 4,
                   False, 304, "an active clip of z"),
    # kappa_sigma = 2 on the trot: clipped rows among the register rows and in the tail
    "clip_trot": (lambda: PlannerConfig.reference_compat(gait="trot", kappa_sigma=2.0), _flat(2, 0, pick=(1, 2)), 4, True, 1156,
                  "an active clip of z on register rows and on tail rows"),
    # a discarded chord step where 132 inequality rows go through memory (the reload of g, the update with al = az = 0 on the
    # tail): the trot on the bilinear exp_5 map under the chord settings above, found among 96 solves on seeds 1 - 11 (seed 6:
    # kinds 0, 0, 2, 0; seed 7: 0, 0, 0, 2, 0 behind a step of three trials)
    "discard_trot": (lambda: PlannerConfig.reference_compat(gait="trot", terrain_mode=0, chord_tol=1e3, chord_shrink=1.0),
                     _picked(((6, 0), (7, 0)), 0), 5, False, 1156, "a discarded chord step on a transcription with a tail"),
}
NAMES = list(CASES)
# transcriptions that only STOPPED runs (no per-step test of their own: the trot's tail is in `trot`, the line searches in bilinear_*)
EXTRA_CASES = {
    # the trot on the bilinear exp_5 map: seed 1 problem 1, seed 2 problem 1
    "bilinear_trot": (lambda: PlannerConfig.reference_compat(gait="trot", terrain_mode=0), _picked(((1, 1), (2, 1)), 0), 4, False, 1156,
                      "jams on a transcription with a tail"),
    # bilinear_1s' problem 0 with its goal 5 m further out: jams under the product's own stall_alpha = 1e-2
    "far_goal": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5, terrain_mode=0),
                 _far(((1, 0),), 0, 5.0), 8, False, 304, "a jam under the product's settings"),
    # max_iter = 0 warm starts whose dual infeasibility is attained by a base coefficient or a force node (see _groups): every
    # other case's is a foothold's or a base-linear unknown's.  Not on the smallest transcription (two_base_polys, 1 s), for two
    # reasons: the reduced base takes effect from 20 base polynomials on (model.hpp), and the coverage has to hold on the
    # reduced system too -- hence the reference transcription, 50 polynomials --; and with the default stance's levers (0.17
    # and 0.2 m) a base-angular unknown collects at most 4 x 0.37 x its B-spline weight (<= 2/3) of the rows' z where a
    # foothold's entry is 1, so a foothold wins the maximum whatever node is moved -- hence the stance 2.5 times as wide
    "groups": (lambda: PlannerConfig.reference_compat(nominal_stance=_wide_stance()), _groups, 0, True, 1024,
               "the dual infeasibility attained by a base-angular, a base-linear and a force unknown"),
}
# The cases on which qo_solve is no reference (its Jacobian pattern comes from one evaluation at a perturbed starting point, see
# bilinear_steps above): on the bilinear trot it parts from the restatement in the FIRST step, by 0.15 to 0.17 in the nodes
# (discard_trot, both bilinear_trot problems; on bilinear_trot 18 and 25 Jacobian entries of iterate 1 are zero at a perturbed
# starting point).  Which of the two takes the Newton step is decided on the GPU: the kernels meet the restatement's dense solve
# of the whole Jacobian at 5e-6 per step on these cases.  Treated as bilinear_no_qo is: the GPU test and the restatement's own
# events only
NO_QO = ("bilinear_no_qo", "discard_trot", "bilinear_trot")
QO_NAMES = [n for n in NAMES if n not in NO_QO]             # the cases on which qo_solve is a reference
DUAL_NAMES = NAMES + ["groups"]                             # the cases of the dual-infeasibility checks (oracle/duals.py)
DISCARD_NAMES = [n for n in NAMES if n.startswith("discard_")]
CLIP_NAMES = [n for n in NAMES if n.startswith("clip_")]
REDUCED_NAMES = [n for n in NAMES if CASES[n][3]]
DUAL_REDUCED_NAMES = REDUCED_NAMES + ["groups"]
# (max_iter: as far as the CPU has run these solves WITHOUT the rules and seen them stay finite -- the GPU test runs them so)
_JAM = dict(stall_iters=0, stall_alpha=0.9, chord_tol=0.0, max_iter=6)
# Solves that the stall or the jam rule stops, and one it must not stop: (case, problem, settings on top of the case's product
# configuration, full system, the stop, the iteration it comes in).  The other problems of a case run along and stop where
# next_kind puts them.
STOPPED = [
    # stalls under the product's settings (stall_iters = 5, stall_alpha = 1e-2, max_iter = 24)
    ("bilinear_steps", 1, {}, "stalled", 9),
    # two short steps at once (alpha 0.062, 0.024; 5 and 6 trials)
    ("bilinear_1s", 3, _JAM, "jammed", 2),
    # the same on 1156 inequality rows, 132 of them through memory (alpha 0.34, 0.18)
    ("bilinear_trot", 0, _JAM, "jammed", 2),
    # a long step first, then the row of two (alpha 0.90, 0.38, 0.046): the counter starts behind a step that does not count
    ("bilinear_trot", 1, _JAM, "jammed", 3),
    # the product's own settings (stall_iters = 5, stall_alpha = 1e-2) on a goal out of reach: alpha ..., 0.0066, 0.00033 while
    # the violation still creeps down (129 -> 104), so the stall rule does not come first
    ("far_goal", 0, dict(max_iter=8), "jammed", 7),
    # discard_bilinear with the jam rule on: alpha 1, 0 (discarded), 0.25, 1, ... -- the discarded step does not count, the
    # counter goes 0, 0, 1, 0 and the solve converges; a counter that took the discarded step would stop it at 3
    ("discard_bilinear", 0, dict(stall_iters=0, stall_alpha=0.9, max_iter=8), "converged", None),
    ("discard_bilinear", 1, dict(stall_iters=0, stall_alpha=0.9, max_iter=8), "converged", None),
]
STALLED = STOPPED[0][:2]                                      # (case, problem) that stalls under the product's settings
# Under the PRODUCT's settings a search on the CPU (oracle/ipm.py's events; 24 trot goals under either mu rule, 12 seeds each of
# step_goals on the bilinear and nearest-cell exp_5 map, both transcriptions, 10 goals of the 100-knot trot, 138 further
# nearest-cell exp_5 solves on the 2.5 s and the reference transcription) found no discarded chord step, no active clip of z and,
# among 56 bilinear solves, four stalls and no jam.  The discard_*, clip_* cases and STOPPED reach all three through settings
# (chord_tol / chord_shrink, kappa_sigma, stall_alpha) and, for the jam, a goal out of reach.  A second search (96 solves of the
# trot on the bilinear and the nearest-cell exp_5 map under chord_tol = 1e3, chord_shrink = 1, seeds 1 - 11, mu_init 0.1, 1, 10,
# kappa_sigma 1e10 and 2) found the discarded chord step on a transcription with a tail 15 times: discard_trot.  Nothing the
# record names is left unfound.
NOT_FOUND = ()

_cache, _runs = {}, {}


class Case:
    pass


def prefix(cfg):
    """The prefix planners run without the stall rules: a stalled or jammed solve hands back its best iterate, not its last."""
    return dataclasses.replace(cfg, stall_iters=0, stall_alpha=0.0)


def case(name):
    if name not in _cache:
        make, inputs, steps, reduced, n_iq, why = CASES[name] if name in CASES else EXTRA_CASES[name]
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
    key = (name, b, None if cfg is None else (cfg.stall_iters, cfg.stall_alpha, cfg.chord_tol, cfg.max_iter))
    if key not in _runs:
        c = case(name)
        _runs[key] = ipm.solve(c.O, c.q[b], cfg or c.cfg_full, x0=None if c.warm is None else c.warm[b], max_iter=None if cfg else c.steps)
    return _runs[key]


def stopped_cfg(entry):
    """The configuration of a STOPPED entry: the case's product configuration on the full system with the entry's settings."""
    return dataclasses.replace(case(entry[0]).product_full, **entry[2])


REDUCED_SETTINGS = ((True, False), (False, True), (True, True))      # (reduce_base, reduce_swing), as test_gpu_linearisation.REDUCED
_bases = {}


def setting(c, key):
    """The case's configuration with (reduce_base, reduce_swing) = key."""
    return dataclasses.replace(c.cfg, reduce_base=key[0], reduce_swing=key[1])


def basis(name, key):
    """(Z, group per column) of oracle/duals.solver_basis for a case under (reduce_base, reduce_swing) = key, cached.  The free
    variables are those of the case's first problem: the same for all of them (asserted by the tests through structure())."""
    if (name, key) not in _bases:
        c = case(name)
        free = ipm.working_set(c.O, c.q[0])[0]
        _bases[(name, key)] = duals.solver_basis(c.O, c.O.L, setting(c, key), free)
    return _bases[(name, key)]


def entry_gate(c):
    """The gate on a Jacobian entry: the bilinear map's slopes of 2.7 enter its entries."""
    return lc.GATE_ENTRY_BILINEAR if c.cfg.terrain_mode == 0 else GATE_ENTRY


def dual_measure(c, Z, x, y, zl, zu, J=None):
    """The restatement's dual infeasibility at nodes x with y, z_l, z_u by constraint row, on the case's terrain: (value, attaining
    column, gate).  The gate, derived like item 3 of test_gpu_steps.py's header and from no measured number: the product forms
    per unknown p the sum over its Jacobian entries of G_rp v_r, G the entries of J Z as its linearisation wrote them, each off
    by at most the gate on an entry times the weight |Z| of the node variables behind it -- GATE_ENTRY sum |Z| |v| --, and
    summed in float64 in another order than here: (terms + 4) u sum |Z| |J| |v| (the four: forming v = y + z_u - z_l and
    the products' own roundings).  The largest over the columns: the maximum of two lists whose entries differ by at most their
    bounds differs by at most the largest bound."""
    val, col, info = duals.dual_infeasibility(c.O.jacobian(x) if J is None else J, Z, y, zl, zu)
    return val, col, dual_gate(info, entry_gate(c))


def dual_gate(info, gate_entry):
    """The gate of dual_measure from the per-column figures of duals.dual_infeasibility."""
    return float((gate_entry * info["weight"] + (info["terms"] + 4) * U * info["abs_terms"]).max())


def y_gate_of(spread):
    """The gate on the multipliers y, relative to the dense y's largest entry: GATE_DIRECTION -- dx and y are one solve vector --
    unless ipm.solve_refined and an unrefined LAPACK solve of the same matrix differ by `spread` > GATE_DIRECTION / GATE_FACTOR;
    then GATE_FACTOR times that (the rule kkt_cases uses for GATE_CPU_SPREAD)."""
    return GATE_DIRECTION if spread <= GATE_DIRECTION / lc.GATE_FACTOR else lc.GATE_FACTOR * spread


def record_dual(section, name, entry):
    """Print the figures of a dual-infeasibility check; where the environment variable QTOS_DUAL_ACCURACY names a file, keep them
    in it as JSON (profiles/dual_accuracy.json is such a file from an MI355X run)."""
    print("dual accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_DUAL_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


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
