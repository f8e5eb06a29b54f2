"""Shared by test_linearisation_cpu.py and test_gpu_linearisation.py: the transcriptions the linearisation (eval_all<true> in
csrc/kernels.hpp: constraint values and the Jacobian stream) is checked on, seeded evaluation points away from every trivial
point, the comparison with the oracle, Richardson-extrapolated difference quotients of the oracle's constraints, the accuracy
record.  No tests in here."""
import dataclasses
import json
import os

import numpy as np

from conftest import ROOT  # noqa: F401  (path set-up)

import spline_cases as sc
from oracle import splines as sp
from oracle.oracle import Oracle, oracle_dict
from qtos_amd.config import PlannerConfig

# The cases and the path of eval_all / Symbolic::build_linear_terms each is there for.  n_dyn_times, n_rom_times are those of
# capi.analyze without the reduced system; test_the_case_table_sits_on_the_paths_it_names holds them to these figures.
CASES = {
    # the anchor: the transcription of the two Jacobian tests of test_gpu_parity.py (1040 x 1730)
    "walk": (lambda: PlannerConfig.reference_compat(), 52, 64),
    # the other phase tables; the numbers of force and terrain instances are no multiples of the thread count (1280 x 1934)
    "trot": (lambda: PlannerConfig.reference_compat(gait="trot"), 52, 64),
    # one dynamics chunk whose count is no whole number of waves: cpad = 128 > cnt = 102 (1880 x 2534)
    "knots100_trot": (lambda: PlannerConfig.knots100(gait="trot"), 102, 64),
    # the smallest 0.05 s transcription with two dynamics chunks, 2 x 65 knots: the c0 > 0 pass, dyn_t1_off / dyn_t3_off of a
    # second chunk, cpad = 128 > cnt = 65 (1976 x 2882; planner creation accepts it without the reduced base, front 144)
    "two_dyn_chunks": (lambda: PlannerConfig(duration=6.4, dt_base=0.05, dt_dynamic=0.05), 130, 82),
    # what the mpc_random workload runs: 2 x 101 knots, 508 range-of-motion instances -- four short of a second chunk --, the
    # start velocities among the fixed variables (3160 x 4558)
    "knots200_vel": (lambda: PlannerConfig.knots200(honor_start_velocity=True), 202, 127),
    # 608 range-of-motion instances in two chunks of 304, the dynamics knots in one (1880 x 3626)
    "two_rom_chunks": (lambda: PlannerConfig.reference_compat(duration=12.0), 122, 152),
    # a last base polynomial shorter than the rest: 12 x 0.2 s + 0.1 s (596 x 908)
    "short_last_poly": (lambda: PlannerConfig(duration=2.5, dt_base=0.2, dt_dynamic=0.2), 14, 33),
    # fewer items than threads in every section of eval_all (464 x 434)
    "two_base_polys": (lambda: PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5), 4, 4),
}
NAMES = list(CASES)
DYN_CHUNK_MAX, ROM_CHUNK_MAX = 128, 512                    # Symbolic::build_linear_terms
TWO_DYN_CHUNKS = {"two_dyn_chunks", "knots200_vel"}       # n_dyn_times > 128
TWO_ROM_CHUNKS = {"two_rom_chunks"}                       # 4 n_rom_times > 512

# Whether the coefficients of the term lists sit in LDS (DevPlan::coef_in_lds: they do where the evaluation scratch plus
# 8 bytes per DISTINCT coefficient stay within 150 KiB).  The count of distinct coefficients is formed at planner creation and
# no entry point reports it: not determined for any case.  lds_room() gives the part that can be worked out, the
# coefficients that would still fit.
COEF_IN_LDS = {name: "not determined" for name in CASES}

GATE_VALUE = GATE_ENTRY = 1e-10        # test_gpu_parity.py: constraint values / Jacobian entries
GATE_ENTRY_BILINEAR = 1e-9             # test_gpu_parity.py, the terrain test: slopes of 2.7 enter
GATE_FACTOR = sc.GATE_FACTOR           # a gate measured on the reference = its floor times this

NOISE_MOTION, NOISE_EULER, NOISE_FORCE = 0.05, 0.2, 5.0
FD_STEP = 2.0 ** -10                   # flat ground
FD_STEP_TERRAIN = 2.0 ** -14           # bilinear map: 2 h = 1.2e-4 of a 9.1e-3 cell on either side of a grid line
FD_ALL_COLUMNS_UP_TO, FD_SAMPLE = 1300, 400
FOOTHOLD_SPREAD = 0.3                  # as test_terrain_constraints_and_jacobian_match_oracle: the footholds over the ledges
# seeds of points(name, 1, seed, spread) with every foot's x and y further than 2 h from a grid line of exp5_terrain()
TERRAIN_FD_SEED = {"walk": 4, "trot": 98}

_cache = {}


def full(cfg):
    """cfg with every row of the reference's NLP in the KKT system: the system whose Jacobian debug_eval hands out."""
    return dataclasses.replace(cfg, reduce_base=False, reduce_swing=False)


def case(name):
    """(cfg as the table has it -- the reduced system on --, Oracle on flat ground, layout), built once."""
    if name not in _cache:
        cfg = CASES[name][0]()
        _cache[name] = (cfg, Oracle(oracle_dict(cfg)), sp.layout(cfg))
    return _cache[name]


def lds_room(name):
    """Distinct coefficients that fit into LDS next to the scratch of the full system's evaluation kernels (qtos_planner.hip:
    n_sol doubles of nodes, the local Jacobians and the pre-evaluated inputs of one chunk; DYN_LOC = 54, ROM_LOC = 18,
    DYN_VIN = 39, ROM_VIN = 9)."""
    cfg, O, _ = case(name)
    n_dyn, n_rom = O.L.n_dyn_times, 4 * O.L.n_rom_times
    dc = -(-n_dyn // max(1, -(-n_dyn // DYN_CHUNK_MAX)))
    rc = -(-n_rom // max(1, -(-n_rom // ROM_CHUNK_MAX)))
    scratch = (O.n + 1) // 2 * 2 + max(54 * dc, 18 * rc) + max(39 * dc, 9 * rc)
    return 150 * 1024 // 8 - scratch


def noise_sigma(L):
    """0.05 on the motion variables, 0.2 on the nodes of the Euler-angle spline, 5 on the force nodes."""
    return np.where(L.var_set >= 6, NOISE_FORCE, np.where(L.var_set == 1, NOISE_EULER, NOISE_MOTION))


def foot_motion(L):
    """Mask of the feet's motion variables."""
    return (L.var_set >= 2) & (L.var_set < 6)


def fixed(name):
    """Mask of the fixed variables of a case."""
    return case(name)[2].fix_src >= 0


def points(name, n, seed, spread=0.0, sigma=None):
    """n evaluation points of a case, each its own: the oracle's straight-line guess of a seeded problem plus seeded noise --
    large enough that an index error is an error of the first order and that every rotation block of the Jacobian matters --,
    the fixed variables back on their bounds.  spread (terrain): the problems start at x = 0, 0.05, ... and the feet's motion
    variables are moved by `spread`, which puts the footholds on the ledges of the exp_5 map (x = 0.31 .. 1.5).
    Returns (x [n, n_vars], start [n, 24], goal [n, 3])."""
    cfg, O, L = case(name)
    start, goal = sc.problems(n, seed)
    if spread:
        shift = start[:, 0] - 0.05 * np.arange(n)
        start[:, [0, 6, 9, 12, 15]] -= shift[:, None]
        goal[:, 0] -= shift
    rng = np.random.default_rng(seed + 2000)
    qs = [sc.oracle_problem(O, cfg, start[b], goal[b]) for b in range(n)]
    x = np.stack([O.initial_guess(q) for q in qs])
    x += rng.normal(size=x.shape) * (noise_sigma(L) if sigma is None else sigma)
    x[:, foot_motion(L)] += spread
    for b, q in enumerate(qs):
        lo, hi = O.var_bounds(q)
        fx = lo == hi
        assert np.array_equal(fx, fixed(name))
        x[b, fx] = lo[fx]
    return x, start, goal


def mask_jacobian(Jo, fx, row_kind):
    """The oracle's Jacobian as debug_eval hands it out: fixed columns and rows of kind 0 are zero."""
    Jo = Jo.copy()
    Jo[:, fx] = 0
    Jo[row_kind == 0] = 0
    return Jo


def compare(g, J, go, Jo, pattern=False):
    """Largest absolute differences of constraint values and Jacobian entries; pattern: and whether the two Jacobians have
    their non-zeros in the same places."""
    out = dict(values=float(np.abs(np.asarray(g) - go).max()), entries=float(np.abs(np.asarray(J) - Jo).max()))
    if pattern:
        out["pattern_equal"] = bool(np.array_equal(np.asarray(J) != 0, Jo != 0))
    return out


def fd_columns(name, seed=0):
    """The columns of a case's flat-ground difference quotients: all up to 1300 variables, else a seeded sample of 400 with
    every variable set (base linear, base angular, each foot's motion, each foot's force) and both values and derivatives."""
    L = case(name)[2]
    if L.n_vars <= FD_ALL_COLUMNS_UP_TO:
        return np.arange(L.n_vars)
    rng = np.random.default_rng(seed)
    key = 2 * L.var_set + L.var_is_vel
    cols = [int(rng.choice(np.nonzero(key == k)[0])) for k in np.unique(key)]
    rest = np.setdiff1d(np.arange(L.n_vars), cols)
    cols += rng.choice(rest, FD_SAMPLE - len(cols), replace=False).tolist()
    return np.sort(np.array(cols))


def richardson(O, x, cols, h):
    """(R(h), R(h/2)) [n_cons, len(cols)]: central difference quotients D of O.constraints at x, Richardson-extrapolated,
    R(h) = (4 D(h/2) - D(h)) / 3.  Differences and quotients in np.longdouble, over the step the two arguments really
    differ by."""
    def D(c, s):
        xp, xm = x.copy(), x.copy()
        xp[c] += s
        xm[c] -= s
        return (O.constraints(xp).astype(np.longdouble) - O.constraints(xm)) / (np.longdouble(xp[c]) - np.longdouble(xm[c]))
    R1, R2 = np.empty((O.m, len(cols)), np.longdouble), np.empty((O.m, len(cols)), np.longdouble)
    for k, c in enumerate(cols):
        d1, d2, d4 = D(c, h), D(c, h / 2), D(c, h / 4)
        R1[:, k] = (4 * d2 - d1) / 3
        R2[:, k] = (4 * d4 - d2) / 3
    return R1, R2


def fd_check(O, x, cols, h):
    """The oracle's Jacobian at x against R(h) on the given columns.  Returns (floor, gate, achieved): the floor is the
    difference quotients' own disagreement at two step sizes, max |R(h) - R(h/2)|, the gate GATE_FACTOR times it."""
    R1, R2 = richardson(O, x, cols, h)
    floor = float(np.abs(R1 - R2).max())
    return floor, GATE_FACTOR * floor, float(np.abs(O.jacobian(x)[:, cols] - R1).max())


def grid_clearance(name, x, cell, x0=-1.0, y0=-1.0):
    """Smallest distance of any foot's x or y at the point x from a grid line of a heightfield (the kinks of the bilinear
    surface)."""
    L = case(name)[2]
    best = np.inf
    for d, o in ((0, x0), (1, y0)):
        v = (x[foot_motion(L) & (L.var_is_vel == 0) & (L.var_dim == d)] - o) / cell
        best = min(best, float(np.abs(v - np.round(v)).min()) * cell)
    return best


def record(section, name, entry):
    """Print a check's figures; where the environment variable QTOS_LINEARISATION_ACCURACY names a file, keep them in it as
    JSON (profiles/linearisation_accuracy.json is such a file from an MI355X run)."""
    print("linearisation accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_LINEARISATION_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
