"""ctypes binding of the HIP planner library (csrc/libqtos_planner.so, ABI in include/qtos_planner.h).

The header's mirror -- constants, structures, prototypes -- is abi.py and is re-exported here; this module adds the builders of
the parameter structures, the host-only analyses and ``Planner``, the owning wrapper of a handle.

There is no CPU fallback: if the library is missing or no MI355X is visible, loading / creating a
planner raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C quadruped-trajectory-optimization-stack_amd/csrc``.
"""
import ctypes as C
import os

import numpy as np

from .abi import *  # noqa: F401,F403  (the mirror is part of this module's interface: capi.QtosTrack, capi.TRACK_COLS, capi.EXPORTS ...)
from .abi import (CHECK_ACCUMULATE, CHECK_COLS, CHECK_FAMILIES, CSV_COLS, FEEDBACK_QUAT, FEEDBACK_SNAP, FEEDBACK_ZERO_FILTER,
                  FIT_ACCUMULATE, FIT_COLS, FIT_FAMILIES, QP_COLS, HIST_COLS, JOINT_NO_FF, MAX_PHASES, NEE, PROTOTYPES, ROLLOUT_COLS,
                  ROLLOUT_FEET_COLS, ROLLOUT_INIT, ROLLOUT_QP_COLS, ROLLOUT_QUAT, ROLLOUT_STATE, START_DOUBLES, TRACK_CLEAN_DELAY, TRACK_COLS, TRACK_QUAT, QtosDims,
                  QtosForceFit, QtosForceQp, QtosHandover, QtosJointRows, QtosFeedback, QtosParams, QtosPathGoal, QtosPathPlan, QtosPlanCheck,
                  QtosProbe, QtosReport, QtosRollout, QtosRolloutFeet, QtosRolloutQp, QtosSelftest, QtosStitch, QtosTerrainEnv, QtosTrack)

_HERE = os.path.dirname(os.path.abspath(__file__))
# (QTOS_LIB names another build of the library in csrc/: A/B timing of kernel variants, scratch/ab2.py)
LIB_PATH = os.path.join(_HERE, "csrc", os.environ.get("QTOS_LIB", "libqtos_planner.so"))

HIST_NAMES = ("inf_pr", "theta", "mu", "dnorm", "alpha_pr", "alpha_du", "ls", "kind", "compl", "inf_du")
HANDOVER_RULES = {"force": 0, "heights": 1}
STITCH_MODES = {"clean": 0, "reference": 1}     # first_row of the two modes of stitcher.Stitcher
PATH_BASES = {"spine": 0, "state": 1}           # base point of the clipped step: Global_Planner.update / plan_init
CHECK_TOL = (1e-3, 1e-2, 1e-4, 1e-4, 1e-2)      # check_params' default per family: N m, N, m, m, N
FIT_TOL = (1e-3, 1e-2, 5.0, 1e-2)               # fit_params' default per family (force_fit.FIT_TOL): N m, N, N, N
MAX_TRIED = 3                                   # order rules 0, 1, 2


# ---- builders of the parameter structures ----
def _leg(g, robot):
    """The leg block of a parameter structure from a robot (joints.SOLO12, or a structure that carries the block): hip, lateral
    and the link lengths, and knee_sign where the structure has it."""
    for e in range(4):
        for d in range(3):
            g.hip[e][d] = float(robot.hip[e][d])
        g.lateral[e] = float(robot.lateral[e])
        if hasattr(g, "knee_sign"):
            g.knee_sign[e] = float(robot.knee_sign[e])
    g.l_upper, g.l_lower = float(robot.l_upper), float(robot.l_lower)


def _map_shape(maps, name="map_yx", first="n_maps"):
    """(n_maps, rows, cols) of maps given as n_maps x rows x cols or rows x cols (an array, a tensor or nested lists), or as
    that shape (a tuple or list of 2 or 3 ints)."""
    is_shape = isinstance(maps, (tuple, list)) and len(maps) in (2, 3) and all(isinstance(v, (int, np.integer)) for v in maps)
    shape = tuple(int(v) for v in (maps if is_shape else np.shape(maps)))
    if len(shape) not in (2, 3):
        raise ValueError("%s is %s x rows x cols or rows x cols, or that shape" % (name, first))
    return (1,) + shape if len(shape) == 2 else shape


def handover_params(advance=2.5, search=0.4, hz=1000.0, rule="force", heights=(0.0,), zero_filter=False, x_range=None):
    """A QtosHandover: rule "force" (all four f_z > 0) or "heights" (every foot's z, at 6 decimals, in `heights`: Combiner._state)."""
    h = QtosHandover()
    h.advance, h.search, h.hz = float(advance), float(search), float(hz)
    h.rule = HANDOVER_RULES[rule] if isinstance(rule, str) else int(rule)
    hs = [float(v) for v in heights] if h.rule == 1 else []
    if len(hs) > 8:
        raise ValueError("at most 8 terrain heights")
    h.n_heights = len(hs)
    for i, v in enumerate(hs):
        h.heights[i] = v
    h.zero_filter = int(bool(zero_filter))
    h.turn = int(x_range is not None)
    if x_range is not None:
        h.x_lo, h.x_hi = float(x_range[0]), float(x_range[1])
    return h


def stitch_params(capacity, first_row=0, n_rows=0, hz=1000.0, advance_clock=True):
    """A QtosStitch: rows first_row .. first_row + n - 1 of every window's plan go to its ring of `capacity` rows; first_row 0
    ("clean") or 1 ("reference": pd.read_csv eats row 0, Stitcher(mode="reference"))."""
    s = QtosStitch()
    s.hz, s.capacity = float(hz), int(capacity)
    s.first_row = STITCH_MODES[first_row] if isinstance(first_row, str) else int(first_row)
    s.n_rows, s.advance_clock = int(n_rows), int(bool(advance_clock))
    return s


def path_goal_params(horizon=5.0, step_size=1.0, tol=1e-5, z_offset=0.24, cell=0.1, origin=(1.0, 1.0), t_stop=5.0, stop_dist=0.0,
                     base="spine", clamp_x=False, advance_clock=True, hold_done=False, table=None, map_yx=None):
    """A QtosPathGoal with the reference's constants as defaults; base "spine" (Global_Planner.update) or "state" (plan_init,
    spine_step(com, t)).  table (global_planner.path_table) and map_yx (n_maps x rows x cols, or rows x cols) fill the sizes."""
    g = QtosPathGoal()
    g.horizon, g.step_size, g.tol, g.z_offset = float(horizon), float(step_size), float(tol), float(z_offset)
    g.cell, g.origin_x, g.origin_y = float(cell), float(origin[0]), float(origin[1])
    g.t_stop, g.stop_dist = float(t_stop), float(stop_dist)
    g.base = PATH_BASES[base] if isinstance(base, str) else int(base)
    g.clamp_x, g.advance_clock, g.hold_done = int(bool(clamp_x)), int(bool(advance_clock)), int(bool(hold_done))
    if table is not None:
        g.n_paths, g.max_pieces = (int(v) for v in np.shape(table["coef"])[0::3])
    if map_yx is not None:
        g.n_maps, g.rows, g.cols = _map_shape(map_yx)
    return g


def path_plan_params(step_size=1.0, cell=0.1, origin=(1.0, 1.0), height_bound=0.2, max_cells=None, max_open=4096, max_pieces=None,
                     set_done=False, bool_map=None):
    """A QtosPathPlan with the reference's constants as defaults.  bool_map (n_maps x rows x cols, or rows x cols) fills the
    sizes; max_cells defaults to 2 * max_pieces, or without max_pieces to 2 * (rows + cols), twice the longest way across an
    empty grid; max_pieces defaults to what max_cells needs, (max_cells + 1) // 2."""
    g = QtosPathPlan()
    g.step_size, g.cell, g.origin_x, g.origin_y = float(step_size), float(cell), float(origin[0]), float(origin[1])
    g.height_bound, g.max_open, g.set_done = float(height_bound), int(max_open), int(bool(set_done))
    if bool_map is not None:
        g.n_maps, g.rows, g.cols = _map_shape(bool_map, "bool_map")
    if max_cells is None:
        max_cells = min(2 * (g.rows + g.cols), 16384) if max_pieces is None else 2 * int(max_pieces)
    g.max_cells = int(max_cells)
    g.max_pieces = (g.max_cells + 1) // 2 if max_pieces is None else int(max_pieces)
    return g


def probe_params(map_yx=None, multi_map_shift=1, scale=1, origin_shift=1.0, cell=0.1, z_offset=0.24,
                 nominal_stance=((0.21, 0.19, 0.0), (0.21, -0.19, 0.0), (-0.21, 0.19, 0.0), (-0.21, -0.19, 0.0))):
    """A QtosProbe with the reference's constants as defaults (feasibility.probe_table's).  map_yx fills the sizes: the maps
    (n_maps x rows x cols, or rows x cols; an array, a tensor or nested lists) or their shape (a tuple or list of 2 or 3 ints)."""
    g = QtosProbe()
    g.cell, g.scale, g.multi_map_shift = float(cell), int(scale), int(multi_map_shift)
    g.origin_shift, g.z_offset = float(origin_shift), float(z_offset)
    for e in range(NEE):
        for k in range(3):
            g.nominal_stance[e][k] = float(nominal_stance[e][k])
    if map_yx is not None:
        g.n_maps, g.rows, g.cols = _map_shape(map_yx)
    return g


def terrain_env_params(base_yx=None, n_maps=None, n_shift=10, n_height=10, climb=False, delta=0.005):
    """A QtosTerrainEnv with the reference's constants as defaults (n_shift: 10 * mesh_scale there).  base_yx fills the sizes: the
    base grids (n_base x rows x cols, or rows x cols) or their shape; n_maps: None = one map per base grid."""
    g = QtosTerrainEnv()
    g.n_shift, g.n_height, g.climb, g.delta = int(n_shift), int(n_height), int(bool(climb)), float(delta)
    if base_yx is not None:
        g.n_base, g.rows, g.cols = _map_shape(base_yx, "base_yx", "n_base")
        g.n_maps = g.n_base
    if n_maps is not None:
        g.n_maps = int(n_maps)
    return g


def joint_params(hz=1000.0, first_row=0, n_rows=0, capacity=0, ee_shift=0.015, kp=20.0, kd=0.08, hip_scale=1.0, knee_scale=1.0,
                 ankle_scale=1.0, tau_max=8.0, feed_forward=True, robot=None):
    """A QtosJointRows with the SOLO12 leg (joints.SOLO12), towr_transform's ee_shift and the gains of the reference's
    data/config/solo12.yml (kp 20, kd 0.08, scales 1, t_max 8) as defaults.  capacity 0: table mode."""
    from . import joints
    g = QtosJointRows()
    g.hz, g.first_row, g.n_rows, g.capacity, g.ee_shift = float(hz), int(first_row), int(n_rows), int(capacity), float(ee_shift)
    _leg(g, joints.SOLO12 if robot is None else robot)
    for j, (a, b) in enumerate(zip(*joints.motor_gains(kp, kd, hip_scale, knee_scale, ankle_scale))):
        g.kp[j], g.kd[j] = float(a), float(b)
    g.tau_max = float(tau_max)
    g.flags = 0 if feed_forward else JOINT_NO_FF
    return g


def track_params(hz=1000.0, first_row=0, n_rows=0, capacity=0, ee_shift=0.015, delay=500, rule="reference", quaternion=False, robot=None):
    """A QtosTrack with the SOLO12 leg (joints.SOLO12), towr_transform's ee_shift and the reference's delay of 500 calls as
    defaults.  rule: "reference" (Tracking.update's branches as they stand) or "clean" (recorded iff call > delay); quaternion: the
    measured rows carry (x, y, z, w) instead of Euler angles.  capacity 0: table mode."""
    from . import joints, tracking
    if rule not in tracking.RULES:
        raise ValueError("rule is 'reference' or 'clean'")
    g = QtosTrack()
    g.hz, g.first_row, g.n_rows, g.capacity, g.ee_shift = float(hz), int(first_row), int(n_rows), int(capacity), float(ee_shift)
    _leg(g, joints.SOLO12 if robot is None else robot)
    g.delay = int(delay)
    g.flags = (TRACK_QUAT if quaternion else 0) | (TRACK_CLEAN_DELAY if rule == "clean" else 0)
    return g


def feedback_params(cfg=None, hz=1000.0, first_row=0, n_rows=0, capacity=0, latency=0.0, gain_pos=1.0, gain_ang=1.0, gain_foot=1.0,
                    max_pos=0.05, max_ang=0.2, max_foot=0.05, snap=True, zero_filter=False, quaternion=False, robot=None, ee_shift=0.015,
                    nominal=None, max_deviation=None, rom_tol=1e-6, snap_tol=0.02):
    """A QtosFeedback with the SOLO12 leg (joints.SOLO12), towr_transform's ee_shift, full gains, clips of 0.05 m / 0.2 rad /
    0.05 m and the snap as defaults.  cfg: the planner's PlannerConfig (None: the defaults'), which gives the range-of-motion
    box, nominal and max_deviation, unless those are given.  capacity 0: table mode."""
    from . import joints
    from .config import PlannerConfig
    cfg = PlannerConfig() if cfg is None else cfg
    nominal = cfg.nominal_stance if nominal is None else nominal
    max_deviation = cfg.max_deviation if max_deviation is None else max_deviation
    g = QtosFeedback()
    g.hz, g.first_row, g.n_rows, g.capacity, g.latency = float(hz), int(first_row), int(n_rows), int(capacity), float(latency)
    g.ee_shift = float(ee_shift)
    _leg(g, joints.SOLO12 if robot is None else robot)
    for e in range(4):
        for d in range(3):
            g.nominal[e][d] = float(nominal[e][d])
    g.gain_pos, g.gain_ang, g.gain_foot = float(gain_pos), float(gain_ang), float(gain_foot)
    g.max_pos, g.max_ang, g.max_foot = float(max_pos), float(max_ang), float(max_foot)
    for d in range(3):
        g.max_deviation[d] = float(max_deviation[d])
    g.rom_tol, g.snap_tol = float(rom_tol), float(snap_tol)
    g.flags = (FEEDBACK_QUAT if quaternion else 0) | (FEEDBACK_SNAP if snap else 0) | (FEEDBACK_ZERO_FILTER if zero_filter else 0)
    return g


def check_params(hz=1000.0, first_row=0, n_rows=0, tol=CHECK_TOL, accumulate=False):
    """A QtosPlanCheck.  tol: one number for the five families (dyn_ang N m, dyn_lin N, rom m, terrain m, force N) or five."""
    g = QtosPlanCheck()
    g.hz, g.first_row, g.n_rows = float(hz), int(first_row), int(n_rows)
    for f, v in enumerate(np.broadcast_to(np.asarray(tol, np.float64), (CHECK_FAMILIES,))):
        g.tol[f] = float(v)
    g.flags = CHECK_ACCUMULATE if accumulate else 0
    return g


def fit_params(cfg=None, hz=1000.0, first_row=0, n_rows=0, capacity=0, tol=FIT_TOL, accumulate=False, **kw):
    """A QtosForceFit from force_fit.fit_params(cfg, **kw) -- arm, damping, w_min, excess_tol, robot, ee_shift with its defaults and
    its checks (ValueError).  tol: one number for the four families (res_ang N m, res_lin N, change N, excess N) or four.
    capacity 0: table mode."""
    from . import force_fit
    r = force_fit.fit_params(cfg, **kw)
    g = QtosForceFit()
    g.hz, g.first_row, g.n_rows, g.capacity = float(hz), int(first_row), int(n_rows), int(capacity)
    g.flags = FIT_ACCUMULATE if accumulate else 0
    g.arm, g.damping, g.w_min, g.excess_tol = r.arm, r.damping, r.w_min, r.excess_tol
    for f, v in enumerate(np.broadcast_to(np.asarray(tol, np.float64), (FIT_FAMILIES,))):
        g.tol[f] = float(v)
    _leg(g, r)
    g.ee_shift = r.ee_shift
    return g


def qp_params(cfg=None, hz=1000.0, first_row=0, n_rows=0, capacity=0, tol=FIT_TOL, accumulate=False, **kw):
    """A QtosForceQp from force_qp.qp_params(cfg, **kw) -- mu, f_max (None: cfg's friction and force_limit), mu_end, act_tol,
    max_iter and the fit's arm, damping, w_min, robot, ee_shift, with their defaults and checks (ValueError).  tol: one number for
    the four families (res_ang N m, res_lin N, change N, limited N) or four.  capacity 0: table mode."""
    from . import force_qp
    r = force_qp.qp_params(cfg, **kw)
    g = QtosForceQp()
    g.hz, g.first_row, g.n_rows, g.capacity = float(hz), int(first_row), int(n_rows), int(capacity)
    g.flags = FIT_ACCUMULATE if accumulate else 0
    g.arm, g.damping, g.w_min, g.excess_tol = r.arm, r.damping, r.w_min, r.excess_tol
    for f, v in enumerate(np.broadcast_to(np.asarray(tol, np.float64), (FIT_FAMILIES,))):
        g.tol[f] = float(v)
    _leg(g, r)
    g.ee_shift = r.ee_shift
    g.mu, g.f_max, g.mu_end, g.act_tol, g.max_iter = r.mu, r.f_max, r.mu_end, r.act_tol, r.max_iter
    return g


def rollout_params(cfg=None, hz=1000.0, substeps=1, first_row=0, n_rows=0, capacity=0, init=False, quaternion=False, mass=None,
                   gravity=None, inertia_b=None, ff_scale=1.0, kp_lin=0.0, kd_lin=0.0, kp_ang=0.0, kd_ang=0.0, f_fb_max=0.0,
                   t_fb_max=0.0, dev_max=0.0, tilt_max=0.0, push_from=0, push_ticks=0):
    """A QtosRollout.  cfg: the planner's PlannerConfig (None: the defaults'), which gives mass, gravity and inertia_b unless
    those are given; the inertia is inverted here, in float64 (a singular one raises ValueError).  The gains are one number
    for the three world axes or three; the defaults are an open loop without limits.  capacity 0: table mode."""
    from . import rollout
    r = rollout.RolloutParams(cfg, mass, gravity, inertia_b, substeps, ff_scale, kp_lin, kd_lin, kp_ang, kd_ang, f_fb_max, t_fb_max,
                              dev_max, tilt_max, push_from, push_ticks, quaternion)
    g = QtosRollout()
    g.hz, g.substeps, g.first_row, g.n_rows, g.capacity = float(hz), r.substeps, int(first_row), int(n_rows), int(capacity)
    g.flags = (ROLLOUT_INIT if init else 0) | r.flags
    g.mass, g.gravity, g.ff_scale = r.mass, r.gravity, r.ff_scale
    for i in range(9):
        g.inertia_b[i], g.inertia_b_inv[i] = float(r.inertia_b[i]), float(r.inertia_b_inv[i])
    for i in range(3):
        g.kp_lin[i], g.kd_lin[i], g.kp_ang[i], g.kd_ang[i] = float(r.kp_lin[i]), float(r.kd_lin[i]), float(r.kp_ang[i]), float(r.kd_ang[i])
    g.f_fb_max, g.t_fb_max, g.dev_max, g.tilt_max = r.f_fb_max, r.t_fb_max, r.dev_max, r.tilt_max
    g.push_from, g.push_ticks = r.push_from, r.push_ticks
    return g


def rollout_feet_params(cfg=None, arm=0.2, damping=1e-6, w_min=0.01, mu=None, f_max=None, limit=False, **body):
    """A QtosRolloutFeet: `body` are rollout_params' keywords (cfg is passed on to it).  arm, damping and w_min default to the fit's,
    mu and f_max to the planner configuration's friction and force limit (cfg None: the defaults'); limit: QTOS_FEET_LIMIT.  A
    value outside its range raises ValueError, as rollout_feet.FeetParams does."""
    from . import rollout_feet
    f = rollout_feet.FeetParams(cfg, arm, damping, w_min, mu, f_max, limit)
    g = QtosRolloutFeet().with_body(rollout_params(cfg=cfg, **body))
    g.arm, g.damping, g.w_min, g.mu, g.f_max, g.feet_flags = f.arm, f.damping, f.w_min, f.mu, f.f_max, f.feet_flags
    return g


def rollout_qp_params(cfg=None, arm=0.2, damping=1e-6, w_min=0.01, mu=None, f_max=None, mu_end=1e-6, act_tol=1e-3, max_iter=25, **body):
    """A QtosRolloutQp: rollout_feet_params' keywords without `limit`, and the QP's mu_end, act_tol and max_iter.  A value outside
    its range raises ValueError, as rollout_qp.QpFeetParams does (mu > 0 and f_max > 0 among them)."""
    from . import rollout_qp
    f = rollout_qp.QpFeetParams(cfg, arm, damping, w_min, mu, f_max, mu_end, act_tol, max_iter)
    g = QtosRolloutQp().with_body(rollout_params(cfg=cfg, **body))
    g.arm, g.damping, g.w_min, g.mu, g.f_max, g.feet_flags = f.arm, f.damping, f.w_min, f.mu, f.f_max, 0
    g.mu_end, g.act_tol, g.max_iter = f.mu_end, f.act_tol, f.max_iter
    return g


def params_from_config(cfg):
    p = QtosParams()
    for e in range(NEE):
        d = cfg.phase_durations[e]
        if len(d) > MAX_PHASES:
            raise ValueError("at most %d phases per foot" % MAX_PHASES)
        p.n_phases[e] = len(d)
        for k, v in enumerate(d):
            p.phase_dur[e][k] = float(v)
        for k in range(3):
            p.nominal_stance[e][k] = float(cfg.nominal_stance[e][k])
    p.dt_base, p.dt_dyn, p.dt_rom = cfg.dt_base, cfg.dt_dynamic, cfg.dt_range_of_motion
    p.force_polys_per_stance = cfg.force_polys_per_stance
    p.mass, p.gravity = cfg.mass, cfg.gravity
    for k, v in enumerate(np.asarray(cfg.inertia_b, float).reshape(9)):
        p.inertia_b[k] = v
    for k in range(3):
        p.max_dev[k] = cfg.max_deviation[k]
    p.mu, p.f_max, p.t_swing_avg = cfg.friction, cfg.force_limit, cfg.t_swing_avg
    p.honor_start_velocity = int(cfg.honor_start_velocity)
    p.terrain_mode = int(cfg.terrain_mode)
    p.max_iter, p.tol = cfg.max_iter, cfg.tol
    p.mu_init, p.mu_min, p.delta_x, p.eps_dual = cfg.mu_init, cfg.mu_min, cfg.delta_x, cfg.eps_dual
    p.slack_push = cfg.slack_push
    p.warm_slack_push = cfg.warm_slack_push
    p.stall_iters = cfg.stall_iters
    p.hold_from, p.hold_weight, p.hold_tol = cfg.foothold_hold_from, cfg.foothold_hold_weight, cfg.foothold_hold_tol
    p.chord_tol = cfg.chord_tol
    p.reduce_base = int(cfg.reduce_base)
    p.chord_max, p.chord_shrink = int(cfg.chord_max), float(cfg.chord_shrink)
    p.stall_alpha = float(cfg.stall_alpha)
    p.reduce_swing = int(getattr(cfg, "reduce_swing", False))
    p.mu_superlinear = int(getattr(cfg, "mu_superlinear", False))
    if not float(cfg.kappa_sigma) > 1.0:              # (model.hpp refuses it too: a C caller gets -1, bad parameters)
        raise ValueError("kappa_sigma must be > 1 (Ipopt's default: 1e10), not %r: the clip of z to [mu / (kappa_sigma gap), "
                         "kappa_sigma mu / gap] needs a band to clip to" % (cfg.kappa_sigma,))
    p.kappa_sigma = float(cfg.kappa_sigma)
    return p


class SelftestError(RuntimeError):
    """No elimination order passed the KKT self-test (qtos_planner_create_checked returned -6); `attempts`: the QtosSelftest
    records in the order they were tried."""

    def __init__(self, attempts):
        self.attempts = attempts
        RuntimeError.__init__(self, "no elimination order passed the KKT self-test: " + "; ".join(a.describe() for a in attempts))


# ---- the library ----
_lib = None


def load():
    """Load the HIP library; raises OSError with build instructions if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OSError("HIP planner library not built: %s (run __graft_entry__.build()); "
                      "this package has no CPU fallback" % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 / libhsa-runtime64.  If this library
    # pulled in the system copies first, a later `import torch` would map a second runtime and see no GPU
    # (torch.cuda.is_available() False, RCCL unusable).  Binding to torch's copy -- when torch is installed --
    # makes the import order irrelevant; without torch the system runtime is used.
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        for loc in (spec.submodule_search_locations or []) if spec else []:
            hip = os.path.join(loc, "lib", "libamdhip64.so")
            if os.path.exists(hip):
                C.CDLL(hip, mode=C.RTLD_GLOBAL)
                break
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    _warn_if_two_hip_runtimes()
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name, None)       # (an older build loaded through QTOS_LIB for A/B timing lacks the newer entry points: has())
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    _lib = lib
    return lib


def _warn_if_two_hip_runtimes():
    """The pre-load above gives ONE HIP runtime only if torch's libamdhip64 has the SONAME this library was linked against:
    with a torch wheel built for another ROCm major both copies get mapped and the kernels register with whichever wins
    symbol lookup.  Said loudly instead of failing obscurely later."""
    try:
        paths = {ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}
        real = {os.path.realpath(q) for q in paths}
        if len(real) > 1:
            import warnings
            warnings.warn("two HIP runtimes are mapped into this process (%s): the planner library and PyTorch do not share "
                          "one libamdhip64; GPU work may fail or see no device" % ", ".join(sorted(real)))
    except OSError:
        pass


def has(symbol):
    """Whether the loaded library exports `symbol`."""
    lib = load()
    return hasattr(lib, symbol)


def _need(symbol, what):
    if not has(symbol):
        raise RuntimeError("this build of the planner library has no %s (%s)" % (what, symbol))


# ---- pointers ----
def ptr(t):
    """The device pointer of a tensor for a device form (None stays None)."""
    return None if t is None else t.data_ptr()


def ptr_given(t):
    """ptr() where an argument may also be True or False, which name no tensor."""
    return None if t is None or t is True or t is False else t.data_ptr()


def _dp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int))


def _llp(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_longlong))


def _vp(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- staging of the host forms' arguments (None stays None throughout) ----
def _bcast(a, B, dtype=np.float64, copy=False):
    """A number or an array of B as a contiguous array of B of that dtype; copy: one the call may write to."""
    if a is None:
        return None
    a = np.broadcast_to(np.asarray(a, dtype), (B,))
    return np.array(a) if copy else np.ascontiguousarray(a)


def _vec(a, B, dtype=np.int32):
    """An array of B entries (B -1: of however many it has) as a contiguous one of that dtype."""
    return None if a is None else np.ascontiguousarray(a, dtype).reshape(B)


def _mat(a, shape, copy=False):
    """An array as contiguous float64 of that shape; copy: one the call may write to."""
    return None if a is None else (np.array if copy else np.ascontiguousarray)(a, np.float64).reshape(shape)


def _maps(a):
    """Maps n_maps x rows x cols, or rows x cols for one, as a contiguous float64 array n_maps x rows x cols."""
    a = np.ascontiguousarray(a, np.float64)
    return a[None] if a.ndim == 2 else a


def _rows(params):
    """The rows per window of a window kernel's tables (params.n_rows) or rings (params.capacity)."""
    return int(params.capacity) if params.capacity > 0 else int(params.n_rows)


def _segment(params, B, cursor, *rings):
    """(rows, cursor) of a window kernel's host form: _rows, and the rings' cursor as B contiguous int64 (table mode: None).
    `rings`: what ring mode needs besides."""
    if params.capacity <= 0:
        return _rows(params), None
    if cursor is None or any(r is None for r in rings):
        raise ValueError("ring mode takes the rings as they stand: out, status and cursor" if rings else
                         "ring mode takes the ring's cursor")
    return _rows(params), _bcast(cursor, B, np.int64)


def _table(rows, shape, reshape=False):
    """The `rows` argument of a host form: True: a new table of zeros; False / None: no table; an array: a float64 copy of it
    (reshape: brought to `shape`; otherwise its shape is the caller's to check)."""
    if rows is True:
        return np.zeros(shape)
    if rows is False or rows is None:
        return None
    rows = np.array(rows, np.float64)
    return rows.reshape(shape) if reshape else rows


def _summary(summary, rows, records, B, families):
    """The `summary` argument of a host form: False: none, which needs a table (`rows`); None: empty records; an array: a
    copy of it as B x families records.  records: plan_check or force_fit, which define the dtype SUMMARY."""
    if summary is False:
        if rows is None:
            raise ValueError("rows and summary cannot both be left out")
        return None
    if summary is None:
        return records.empty_summary(B)
    return np.array(summary, records.SUMMARY).reshape(B, families)


def _meas(meas, B, rows, quaternion):
    """The measured rows of a host form as contiguous float64: (B, rows, 18), or 19 columns with the quaternion."""
    mcols = 19 if quaternion else 18
    meas = np.ascontiguousarray(meas, np.float64)
    if meas.shape != (B, max(rows, 0), mcols):
        raise ValueError("meas is (B, %d, %d)" % (rows, mcols))
    return meas


def _out_status(out, status, B, rows, cols):
    """The row table and the status words a host form writes: copies of the arrays as they stand, or (None) zeros."""
    out = np.zeros((B, max(rows, 0), cols)) if out is None else np.array(out, np.float64)
    status = np.zeros((B, max(rows, 0)), np.int32) if status is None else np.array(status, np.int32)
    if out.shape != (B, rows, cols) or status.shape != (B, rows):
        raise ValueError("out is (B, %d, %d) and status (B, %d)" % (rows, cols, rows))
    return out, status


def _goal_pair(goal_step, goal):
    if (goal_step is None) != (goal is None):
        raise ValueError("goal_step and goal go together: give both or neither")


# ---- host-only entry points ----
def build_flags():
    """Bit 0: reserved, always 0; bit 1: stamps; bit 2: development build."""
    return int(load().qtos_build_flags())


def analyze(cfg):
    """Host-only structure analysis: (QtosDims, per-stage populated front sizes).  No GPU needed."""
    lib = load()
    p = params_from_config(cfg)
    d = QtosDims()
    act = np.zeros(4096, np.int32)
    rc = lib.qtos_analyze(C.byref(p), C.byref(d), _ip(act), act.size)
    if rc != 0:
        raise ValueError("qtos_analyze failed (%d)" % rc)
    return d, act[:d.n_stages].copy()


def analyze_counts(cfg):
    """Host-only: (nonzeros of the equality, of the inequality constraint Jacobian) of the full system, the counts the
    Ipopt header prints (qtos_analyze_counts).  None with a library that lacks the entry point."""
    if not has("qtos_analyze_counts"):
        return None
    p = params_from_config(cfg)
    c = (C.c_longlong * 2)()
    if load().qtos_analyze_counts(C.byref(p), c, 2) != 2:
        raise ValueError("qtos_analyze_counts failed")
    return int(c[0]), int(c[1])


def analyze_kernel(cfg):
    """Host-only: the factor + solve kernel a planner created now would select (qtos_analyze_kernel: the name
    Planner.kkt_kernel would report under the current environment)."""
    lib = load()
    p = params_from_config(cfg)
    buf = C.create_string_buffer(64)
    n = lib.qtos_analyze_kernel(C.byref(p), buf, 64)
    if n < 0:
        raise ValueError("qtos_analyze_kernel failed (%d)" % n)
    return buf.value.decode()


def _selftest_lib():
    _need("qtos_planner_selftest", "KKT self-test")
    return load()


def analyze_candidates(cfg, rules_mask=0):
    """Host-only: the order rules a checked create would try, in trial order: a list of (rule, front, stages)."""
    lib = _selftest_lib()
    p = params_from_config(cfg)
    a = [np.zeros(MAX_TRIED, np.int32) for _ in range(3)]
    n = lib.qtos_analyze_candidates(C.byref(p), int(rules_mask), _ip(a[0]), _ip(a[1]), _ip(a[2]), MAX_TRIED)
    if n < 0:
        raise ValueError("qtos_analyze_candidates failed (%d)" % n)
    return [(int(a[0][i]), int(a[1][i]), int(a[2][i])) for i in range(min(n, MAX_TRIED))]


def selftest_inputs(cfg, seed, b):
    """Host-only: (dx0 [n_vars], sig [n_cons], w [n_cons]) of problem b of the self-test with this seed -- what
    Planner.selftest(seed) adds to towr's guess and packs as barrier weights and right-hand side."""
    lib = _selftest_lib()
    p = params_from_config(cfg)
    d, _ = analyze(cfg)
    dx0, sig, w = np.zeros(d.n_vars), np.zeros(d.n_cons), np.zeros(d.n_cons)
    rc = lib.qtos_selftest_inputs(C.byref(p), int(seed), int(b), _dp(dx0), _dp(sig), _dp(w))
    if rc != 0:
        raise ValueError("qtos_selftest_inputs failed (%d)" % rc)
    return dx0, sig, w


def selftest_bits(seed, problem, array, index):
    """The generator's 64-bit word (qtos_selftest_bits; array 0 dx0, 1 sig, 2 w)."""
    return int(_selftest_lib().qtos_selftest_bits(int(seed), int(problem), int(array), int(index)))


def selftest_problem(cfg):
    """Host-only: (start [24], goal [3]) of the self-test's problems."""
    lib = _selftest_lib()
    p = params_from_config(cfg)
    start, goal = np.zeros(START_DOUBLES), np.zeros(3)
    if lib.qtos_selftest_problem(C.byref(p), _dp(start), _dp(goal)) != 0:
        raise ValueError("qtos_selftest_problem failed")
    return start, goal


def analyze_order(cfg):
    """Host-only: the elimination order by position (solver variable, n_sol + row for a multiplier, -1 = dummy pivot)."""
    lib = load()
    p = params_from_config(cfg)
    a = np.full(1 << 15, -2, np.int32)
    n = lib.qtos_analyze_order(C.byref(p), _ip(a), a.size)
    if n < 0 or n > a.size:
        raise ValueError("qtos_analyze_order failed (%d)" % n)
    return a[:n].copy()


def analyze_two_ended(cfg):
    """Host-only: what a two-ended elimination of this model's KKT matrix would look like (qtos_analyze_two_ended): a dict of the
    chain lengths, fronts, the separator and the LDS a workgroup running both chains would need."""
    lib = load()
    p = params_from_config(cfg)
    a = np.zeros(20, np.int32)
    rc = lib.qtos_analyze_two_ended(C.byref(p), _ip(a), a.size)
    if rc != 0:
        raise ValueError("qtos_analyze_two_ended failed (%d)" % rc)
    keys = ("stages_now", "front_now", "split_stage", "stages_left", "stages_right", "sep_unknowns", "stages_sep", "front_left", "front_right",
            "front_sep", "serial_steps", "peak_left", "peak_right", "lds_now", "lds_panels", "lds_records", "lds_cells", "lds_two_chains_as_is",
            "lds_two_chains_lean", "lds_limit")
    return {k: int(v) for k, v in zip(keys, a)}


def analyze_sweep(cfg, max_places=1 << 16):
    """Host-only: the helper waves' schedule of the backward sweep as arrays [rounds, 16]: (rows, entries, pos_min, pos_max)."""
    lib = load()
    p = params_from_config(cfg)
    nr = np.zeros(1, np.int32)
    a = [np.full(max_places, -1, np.int32) for _ in range(4)]
    rc = lib.qtos_analyze_sweep(C.byref(p), _ip(nr), _ip(a[0]), _ip(a[1]), _ip(a[2]), _ip(a[3]), max_places)
    if rc != 0:
        raise ValueError("qtos_analyze_sweep failed (%d)" % rc)
    n = int(nr[0])
    return tuple(x[:16 * n].reshape(n, 16).copy() for x in a)


class Planner:
    """Owning wrapper of a QtosPlanner handle."""

    def __init__(self, cfg, max_batch=256, device=0, checked=False, rules_mask=0, tol_residual=0.0):
        """checked: create through qtos_planner_create_checked -- every candidate order (rules_mask; 0 = those of the automatic
        choice) is built and must pass the KKT self-test; self.selftests keeps the attempts, SelftestError if none passes."""
        self.lib = load()
        self.cfg = cfg
        self.params = params_from_config(cfg)
        self.h = C.c_void_p()
        self.selftests = []
        if checked:
            _selftest_lib()
            tried = (QtosSelftest * MAX_TRIED)()
            n = C.c_int(0)
            rc = self.lib.qtos_planner_create_checked(C.byref(self.params), max_batch, device, int(rules_mask), float(tol_residual),
                                                      C.byref(self.h), tried, MAX_TRIED, C.byref(n))
            self.selftests = [tried[i].copy() for i in range(n.value)]
            if rc == -6:
                raise SelftestError(self.selftests)
            what = "qtos_planner_create_checked"
        else:
            rc = self.lib.qtos_planner_create(C.byref(self.params), max_batch, device, C.byref(self.h))
            what = "qtos_planner_create"
        if rc != 0:
            raise RuntimeError("%s failed (%d): -2 = no HIP device, -3 = out of "
                               "memory, -4 = front too large" % (what, rc))
        self.max_batch, self.device = max_batch, device
        self.init_table = None
        self.dims = QtosDims()
        self.lib.qtos_planner_dims(self.h, C.byref(self.dims))
        self.n, self.m = self.dims.n_vars, self.dims.n_cons

    def close(self):
        if self.h:
            self.lib.qtos_planner_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc, what):
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (what, rc, self.lib.qtos_last_error(self.h).decode()))

    # ---- what this build of the library has (a build loaded through QTOS_LIB for A/B timing may be an older one) ----
    has, _need = staticmethod(has), staticmethod(_need)      # (the module's: a handle's library is the loaded one)

    def has_report(self):
        return self.has("qtos_set_report")

    def has_handover(self):
        return self.has("qtos_handover")

    def has_stitch(self):
        return self.has("qtos_stitch")

    def has_joint_rows(self):
        return self.has("qtos_joint_rows")

    def has_track(self):
        return self.has("qtos_track")

    def has_rollout(self):
        return self.has("qtos_rollout")

    def has_rollout_feet(self):
        return self.has("qtos_rollout_feet")

    def has_rollout_qp(self):
        return self.has("qtos_rollout_qp")

    def has_start_feedback(self):
        return self.has("qtos_start_feedback")

    def has_plan_check(self):
        return self.has("qtos_plan_check")

    def has_force_fit(self):
        return self.has("qtos_force_fit")

    def has_path_goal(self):
        return self.has("qtos_path_goal")

    def has_path_plan(self):
        return self.has("qtos_path_plan")

    def has_probe(self):
        return self.has("qtos_probe")

    def has_terrain_env(self):
        return self.has("qtos_terrain_env")

    def _nodes(self, nodes):
        """(nodes as contiguous float64 B x n, B): how every host form takes its plans."""
        nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, self.n)
        return nodes, nodes.shape[0]

    def set_heightfields(self, maps, cell, x0=-1.0, y0=-1.0):
        """maps: (n_maps, nx, ny) heights, maps[k][ix][iy] at x = x0 + ix*cell, y = y0 + iy*cell."""
        if maps is None:
            self._chk(self.lib.qtos_set_heightfields(self.h, 0, None, 0, 0, 1.0, 0.0, 0.0), "set_heightfields")
            return
        a = _maps(maps)
        self._chk(self.lib.qtos_set_heightfields(self.h, a.shape[0], _dp(a), a.shape[1], a.shape[2],
                                                 cell, x0, y0), "set_heightfields")

    def plan(self, start, goal, map_id=None, warm=None):
        start = _mat(start, (-1, START_DOUBLES))
        goal = _mat(goal, (-1, 3))
        B = start.shape[0]
        nodes = np.empty((B, self.n))
        status = np.empty(B, np.int32)
        iters = np.empty(B, np.int32)
        viol = np.empty(B)
        mid, wm = _vec(map_id, -1), _mat(warm, (B, self.n))
        self._chk(self.lib.qtos_plan_batch(self.h, B, _dp(start), _dp(goal), _ip(mid), _dp(wm),
                                           _dp(nodes), _ip(status), _ip(iters), _dp(viol)), "plan_batch")
        return nodes, status, iters, viol

    # ---- asynchronous form (device pointers): submit / poll / wait, see include/qtos_planner.h ----
    def submit(self, B, d_start, d_goal, d_map_id, d_warm, d_nodes, d_status, d_iters, d_viol, stream):
        """Queue a whole solve on `stream` (raw device pointers / None, stream = hipStream_t as int) and return at once."""
        self._chk(self.lib.qtos_plan_submit(self.h, B, d_start, d_goal, d_map_id, d_warm, d_nodes, d_status, d_iters, d_viol,
                                            C.c_void_p(stream)), "plan_submit")

    def poll(self):
        """True once everything the submitted call needs has been queued (results: synchronise its stream)."""
        done = C.c_int(0)
        self._chk(self.lib.qtos_plan_poll(self.h, C.byref(done)), "plan_poll")
        return bool(done.value)

    def wait(self):
        self._chk(self.lib.qtos_plan_wait(self.h), "plan_wait")

    def set_speculation(self, max_blind_iterations):
        self._chk(self.lib.qtos_set_speculation(self.h, int(max_blind_iterations)), "set_speculation")

    def set_pattern_speculation(self, on):
        """The launch pattern of qtos_plan_submit on / off (off forgets what was learnt)."""
        self._chk(self.lib.qtos_set_pattern_speculation(self.h, int(bool(on))), "set_pattern_speculation")

    def set_kernel_events(self, on):
        """Per-kernel HIP events (what timing() / timing_detail() read) on / off; off = the call's first and last event only."""
        self._chk(self.lib.qtos_set_kernel_events(self.h, int(bool(on))), "set_kernel_events")

    def selftest(self, seed=0, tol_residual=0.0):
        """One run of the KKT self-test on this handle (qtos_planner_selftest): a QtosSelftest; raises while a call is open."""
        self._need("qtos_planner_selftest", "KKT self-test")
        t = QtosSelftest()
        self._chk(self.lib.qtos_planner_selftest(self.h, int(seed), float(tol_residual), C.byref(t)), "planner_selftest")
        return t

    def set_report(self, on):
        """Per-solve report (iteration history + final measures) for the calls submitted from now on; raises while a call is
        open (the flag is latched per call)."""
        self._need("qtos_set_report", "per-solve report")
        self._chk(self.lib.qtos_set_report(self.h, int(bool(on))), "set_report")

    def report(self, b):
        """(QtosReport, history rows [n_rows, HIST_COLS]) of problem b of the last call made with the report on."""
        r = QtosReport()
        rows = np.zeros((self.cfg.max_iter + 1, HIST_COLS))
        n = self.lib.qtos_plan_report(self.h, int(b), C.byref(r), _dp(rows), rows.shape[0])
        if n < 0:
            raise RuntimeError("plan_report failed (%d): %s" % (n, self.lib.qtos_last_error(self.h).decode()))
        return r, rows[:n].copy()

    def duals(self, B):
        """(s, z_l, z_u, y) by constraint row of problems 0 .. B-1 of the last call (qtos_debug_duals)."""
        m = self.dims.n_cons
        out = [np.zeros((B, m)) for _ in range(4)]
        self._chk(self.lib.qtos_debug_duals(self.h, B, *[_dp(a) for a in out]), "qtos_debug_duals")
        return tuple(out)

    def env(self):
        """The environment switches the handle runs with (read once at creation), as a dict of strings."""
        buf = C.create_string_buffer(512)
        self._chk(min(self.lib.qtos_env(self.h, buf, 512), 0), "env")
        return dict(kv.split("=", 1) for kv in buf.value.decode().split())

    def timing_detail(self):
        """Where the time of the last call went (qtos_last_timing_detail): seconds and launch counts."""
        a = (C.c_double * 14)()
        self._chk(self.lib.qtos_last_timing_detail(self.h, a, 14), "last_timing_detail")
        keys = ("total_seconds", "start_seconds", "solve_seconds", "step_seconds", "gap_seconds", "slots", "slots_at_submit",
                "informed_launches", "pattern_calls", "pattern_misses", "kkt_seconds", "kkt_launches", "chord_seconds", "chord_launches")
        return {k: (a[i] if i < 5 or i in (10, 12) else int(a[i])) for i, k in enumerate(keys)}

    def sample(self, nodes, t0, hz=1000.0, n_rows=None):
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        if n_rows is None:
            n_rows = int(round(self.dims.duration * hz)) + 1
        rows = np.empty((B, n_rows, CSV_COLS))
        self._chk(self.lib.qtos_sample_csv(self.h, B, _dp(nodes), _dp(t0), hz, n_rows, _dp(rows)), "sample_csv")
        return rows

    def shift_warm(self, nodes_prev, offset, start, goal, map_id=None):
        """Time-shifted warm start of a replan (qtos_shift_warm): previous plan read `offset` seconds later."""
        nodes_prev, B = self._nodes(nodes_prev)
        off, mid = _bcast(offset, B), _vec(map_id, -1)
        start, goal = _mat(start, (B, START_DOUBLES)), _mat(goal, (B, 3))
        out = np.empty((B, self.n))
        self._chk(self.lib.qtos_shift_warm(self.h, B, _dp(nodes_prev), _dp(off), _dp(start), _dp(goal), _ip(mid), _dp(out)), "shift_warm")
        return out

    def handover(self, nodes, advance=2.5, search=0.4, hz=1000.0, rule="force", heights=(0.0,), zero_filter=False,
                 goal_step=None, goal=None, x_range=None):
        """Hand-over of a replan (qtos_handover, host form): the first of the rows round(advance * hz) .. + round(search * hz)
        of every plan in `nodes` that passes the contact rule.  Returns (start [B, 24], offset [B], row [B]); with goal_step
        (B x 3; turned round outside x_range if that is given) and goal (B x 3; its z is kept) also their new values:
        (start, offset, row, goal_step, goal)."""
        self._need("qtos_handover", "hand-over kernel")
        nodes, B = self._nodes(nodes)
        h = handover_params(advance, search, hz, rule, heights, zero_filter, x_range)
        start, offset, row = np.empty((B, START_DOUBLES)), np.empty(B), np.empty(B, np.int32)
        _goal_pair(goal_step, goal)
        gs, gl = _mat(goal_step, (B, 3), copy=True), _mat(goal, (B, 3), copy=True)
        self._chk(self.lib.qtos_handover(self.h, B, C.byref(h), _dp(nodes), _dp(gs), _dp(start), _dp(gl), _dp(offset), _ip(row)), "handover")
        return (start, offset, row) if gs is None else (start, offset, row, gs, gl)

    def stitch(self, nodes, n_rows, t0, traj, cursor, first_row=0, hz=1000.0, advance_clock=True):
        """Append an executed segment of every plan in `nodes` to its window's ring (qtos_stitch, host form): rows first_row ..
        first_row + n - 1 with n = n_rows[b] (an array: in a loop, the hand-over rows) or n_rows (an int, for every window),
        clamped to 0 .. capacity, go to traj[b][(cursor[b] + j) % capacity]; traj is (B, capacity, 37).  Returns new arrays
        (traj, cursor, t0): cursor + n and, with advance_clock, t0 + n / hz."""
        self._need("qtos_stitch", "stitch kernel")
        nodes, B = self._nodes(nodes)
        traj = np.array(traj, np.float64)
        if traj.ndim != 3 or traj.shape[0] != B or traj.shape[2] != CSV_COLS:
            raise ValueError("traj is (B, capacity, %d)" % CSV_COLS)
        t0, cursor = _bcast(t0, B, copy=True), _bcast(cursor, B, np.int64, copy=True)
        per = None if np.ndim(n_rows) == 0 else _vec(n_rows, B)
        s = stitch_params(traj.shape[1], first_row, 0 if per is not None else n_rows, hz, advance_clock)
        self._chk(self.lib.qtos_stitch(self.h, B, C.byref(s), _dp(nodes), _ip(per), _dp(t0), _dp(traj), _llp(cursor)),
                  "stitch")
        return traj, cursor, t0

    def joint_rows(self, nodes, t0, params=None, first_row=None, n_rows=None, q_mes=None, qd_mes=None, out=None, status=None,
                   cursor=None):
        """Joint rows of every plan in `nodes` (qtos_joint_rows, host form; the rule: joints.joint_rows): 37 columns -- the time
        stamp of the CSV row, q, qdot and tau of the twelve joints -- and an int32 status per row.  params: a QtosJointRows
        (joint_params(); the default: the SOLO12 values at 1 kHz, the whole plan).  Table mode (params.capacity 0): returns
        (rows [B, params.n_rows, 37], status [B, params.n_rows]); row j of window b is joint row first + j, first = first_row[b]
        (an array) or params.first_row.  n_rows (an array) gives every window its own count.  With params.n_rows = 1, first_row
        and the measured q_mes, qd_mes (B x 12) that is one tick of B robots.  Ring mode (params.capacity > 0): `out`
        (B x capacity x 37), `status` (B x capacity) and `cursor` (B) are the rings as they stand; returns new arrays."""
        self._need("qtos_joint_rows", "joint-rows kernel")
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        if params is None:
            params = joint_params(n_rows=int(round(self.dims.duration * 1000.0)) + 1)
        first, per = _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        qm, qdm = _mat(q_mes, (B, 12)), _mat(qd_mes, (B, 12))
        rows, cur = _segment(params, B, cursor, out, status)
        out, status = _out_status(out, status, B, rows, CSV_COLS)
        self._chk(self.lib.qtos_joint_rows(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(first), _ip(per),
                                           _llp(cur), _dp(qm), _dp(qdm), _dp(out), _ip(status)), "joint_rows")
        return out, status

    def track(self, nodes, t0, meas, params, first_row=None, n_rows=None, cursor=None, goal_x=None, count=None, total=None, out=None,
              status=None):
        """Track rows of every plan in `nodes` against the measured states `meas` (qtos_track, host form; the rule:
        tracking.track_rows): 26 columns -- the time stamp of the CSV row, the measured pose as the reference's traj_vec, the five
        errors against the plan's own row, total_com and total_feet after the row -- and an int32 status per row (bit 0 recorded,
        bit 1 reached goal_x, bit 2 gimbal).  params: a QtosTrack (track_params()).  meas is (B, rows, 18), or (B, rows, 19) with
        params' quaternion flag, rows = params.n_rows (table mode) or params.capacity (ring mode: `out`, `status` and `cursor` are
        the rings as they stand, meas is a ring with the same addressing).  count (B, 2) int64 = (calls, recorded) and total (B, 2)
        = (total_com, total_feet) are the accumulators as they stand (None: zeros).  With params.n_rows = 1 and first_row that is
        one tick of B robots.  Returns new arrays (rows, status, count, total)."""
        self._need("qtos_track", "track kernel")
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        first, per = _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        rows = _rows(params)
        meas = _meas(meas, B, rows, params.flags & TRACK_QUAT)
        cur = _segment(params, B, cursor, out, status)[1]
        goal = _bcast(goal_x, B)
        count = np.zeros((B, 2), np.int64) if count is None else np.array(count, np.int64).reshape(B, 2)
        total = np.zeros((B, 2)) if total is None else _mat(total, (B, 2), copy=True)
        out, status = _out_status(out, status, B, rows, TRACK_COLS)
        self._chk(self.lib.qtos_track(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(first), _ip(per),
                                      _llp(cur), _dp(meas), _dp(goal), _llp(count), _dp(total), _dp(out), _ip(status)), "track")
        return out, status, count, total

    def rollout(self, nodes, t0, params, first_row=None, n_rows=None, cursor=None, joint=None, mass_scale=None, push=None, state=None,
                count=None, word=None, meas=None, rows=True, status=None):
        """Roll the windows' bodies out over rows of the plans in `nodes` (qtos_rollout, host form; the rule:
        rollout.rollout_rows).  params: a QtosRollout (rollout_params()).  state (B, 13), count (B) int64 and word (B) int32
        are what the windows carry (None: zeros -- give params the init flag then, or a word of ROLLOUT_PENDING, which sets
        each window on its plan at its own first call with rows).  joint: (B, rows, 37) joint rows whose
        columns 1 .. 12 become the measured joint angles (None: those columns of `meas` stay as they are); mass_scale: a number
        or B; push: (B, 6).  rows = params.n_rows (table mode) or params.capacity (ring mode: `meas`, `rows`, `status` and
        `cursor` are the rings as they stand, joint a ring with the same addressing).  meas: (B, rows, 18), or 19 with params'
        quaternion flag (None: zeros); rows: True, an array (B, rows, 20) or False / None for no table.  Returns new arrays
        (meas, rows or None, status, state, count, word)."""
        self._need("qtos_rollout", "rollout kernel")
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        first, per = _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        nr, cur = _segment(params, B, cursor)
        nr = max(nr, 0)                                    # (a negative n_rows: the library refuses it)
        mcols = 19 if params.flags & ROLLOUT_QUAT else 18
        joint = None if joint is None else np.ascontiguousarray(joint, np.float64)
        if joint is not None and joint.shape != (B, nr, CSV_COLS):
            raise ValueError("joint is (B, %d, %d)" % (nr, CSV_COLS))
        ms, push = _bcast(mass_scale, B), _mat(push, (B, 6))
        state = np.zeros((B, ROLLOUT_STATE)) if state is None else _mat(state, (B, ROLLOUT_STATE), copy=True)
        count = np.zeros(B, np.int64) if count is None else _bcast(count, B, np.int64, copy=True)
        word = np.zeros(B, np.int32) if word is None else _bcast(word, B, np.int32, copy=True)
        meas = np.zeros((B, nr, mcols)) if meas is None else np.array(meas, np.float64)
        rows = _table(rows, (B, nr, ROLLOUT_COLS))
        status = np.zeros((B, nr), np.int32) if status is None else np.array(status, np.int32)
        if meas.shape != (B, nr, mcols) or status.shape != (B, nr) or (rows is not None and rows.shape != (B, nr, ROLLOUT_COLS)):
            raise ValueError("meas is (B, %d, %d), rows (B, %d, %d) and status (B, %d)" % (nr, mcols, nr, ROLLOUT_COLS, nr))
        self._chk(self.lib.qtos_rollout(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(first), _ip(per), _llp(cur), _dp(joint),
                                        _dp(ms), _dp(push), _dp(state), _llp(count), _ip(word), _dp(meas), _dp(rows), _ip(status)),
                  "rollout")
        return meas, rows, status, state, count, word

    def rollout_feet(self, nodes, t0, params, first_row=None, n_rows=None, cursor=None, joint=None, mass_scale=None, push=None, state=None,
                     count=None, word=None, meas=None, rows=True, frows=True, status=None):
        """Roll the windows' bodies out with their feedback delivered through the stance feet (qtos_rollout_feet, host form; the
        rule: rollout_feet.rollout_feet_rows).  params: a QtosRolloutFeet (rollout_feet_params()).  Every other argument is
        rollout()'s; frows: True, an array (B, rows, 16) or False / None for no feet table.  Returns new arrays (meas, rows or None,
        frows or None, status, state, count, word)."""
        self._need("qtos_rollout_feet", "feet rollout kernel")
        body = params
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        first, per = _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        nr, cur = _segment(body, B, cursor)
        nr = max(nr, 0)                                    # (a negative n_rows: the library refuses it)
        mcols = 19 if body.flags & ROLLOUT_QUAT else 18
        joint = None if joint is None else np.ascontiguousarray(joint, np.float64)
        if joint is not None and joint.shape != (B, nr, CSV_COLS):
            raise ValueError("joint is (B, %d, %d)" % (nr, CSV_COLS))
        ms, push = _bcast(mass_scale, B), _mat(push, (B, 6))
        state = np.zeros((B, ROLLOUT_STATE)) if state is None else _mat(state, (B, ROLLOUT_STATE), copy=True)
        count = np.zeros(B, np.int64) if count is None else _bcast(count, B, np.int64, copy=True)
        word = np.zeros(B, np.int32) if word is None else _bcast(word, B, np.int32, copy=True)
        meas = np.zeros((B, nr, mcols)) if meas is None else np.array(meas, np.float64)
        rows, frows = _table(rows, (B, nr, ROLLOUT_COLS)), _table(frows, (B, nr, ROLLOUT_FEET_COLS))
        status = np.zeros((B, nr), np.int32) if status is None else np.array(status, np.int32)
        if meas.shape != (B, nr, mcols) or status.shape != (B, nr) or (rows is not None and rows.shape != (B, nr, ROLLOUT_COLS)) or \
                (frows is not None and frows.shape != (B, nr, ROLLOUT_FEET_COLS)):
            raise ValueError("meas is (B, %d, %d), rows (B, %d, %d), frows (B, %d, %d) and status (B, %d)"
                             % (nr, mcols, nr, ROLLOUT_COLS, nr, ROLLOUT_FEET_COLS, nr))
        self._chk(self.lib.qtos_rollout_feet(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(first), _ip(per), _llp(cur), _dp(joint),
                                             _dp(ms), _dp(push), _dp(state), _llp(count), _ip(word), _dp(meas), _dp(rows), _dp(frows),
                                             _ip(status)), "rollout_feet")
        return meas, rows, frows, status, state, count, word

    def rollout_qp(self, nodes, t0, params, first_row=None, n_rows=None, cursor=None, joint=None, mass_scale=None, push=None, state=None,
                   count=None, word=None, meas=None, rows=True, frows=True, qrows=True, status=None):
        """Roll the windows' bodies out with their stance forces from the pyramid QP (qtos_rollout_qp, host form; the rule:
        rollout_qp.rollout_qp_rows).  params: a QtosRolloutQp (rollout_qp_params()).  Every other argument is rollout_feet()'s;
        qrows: True, an array (B, rows, 8) or False / None for no solve table.  Returns new arrays (meas, rows or None, frows or
        None, qrows or None, status, state, count, word)."""
        self._need("qtos_rollout_qp", "QP rollout kernel")
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        first, per = _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        nr, cur = _segment(params, B, cursor)
        nr = max(nr, 0)                                    # (a negative n_rows: the library refuses it)
        mcols = 19 if params.flags & ROLLOUT_QUAT else 18
        joint = None if joint is None else np.ascontiguousarray(joint, np.float64)
        if joint is not None and joint.shape != (B, nr, CSV_COLS):
            raise ValueError("joint is (B, %d, %d)" % (nr, CSV_COLS))
        ms, push = _bcast(mass_scale, B), _mat(push, (B, 6))
        state = np.zeros((B, ROLLOUT_STATE)) if state is None else _mat(state, (B, ROLLOUT_STATE), copy=True)
        count = np.zeros(B, np.int64) if count is None else _bcast(count, B, np.int64, copy=True)
        word = np.zeros(B, np.int32) if word is None else _bcast(word, B, np.int32, copy=True)
        meas = np.zeros((B, nr, mcols)) if meas is None else np.array(meas, np.float64)
        rows, frows, qrows = _table(rows, (B, nr, ROLLOUT_COLS)), _table(frows, (B, nr, ROLLOUT_FEET_COLS)), _table(qrows, (B, nr, ROLLOUT_QP_COLS))
        status = np.zeros((B, nr), np.int32) if status is None else np.array(status, np.int32)
        if meas.shape != (B, nr, mcols) or status.shape != (B, nr) or (rows is not None and rows.shape != (B, nr, ROLLOUT_COLS)) or \
                (frows is not None and frows.shape != (B, nr, ROLLOUT_FEET_COLS)) or (qrows is not None and qrows.shape != (B, nr, ROLLOUT_QP_COLS)):
            raise ValueError("meas is (B, %d, %d), rows (B, %d, %d), frows (B, %d, %d), qrows (B, %d, %d) and status (B, %d)"
                             % (nr, mcols, nr, ROLLOUT_COLS, nr, ROLLOUT_FEET_COLS, nr, ROLLOUT_QP_COLS, nr))
        self._chk(self.lib.qtos_rollout_qp(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(first), _ip(per), _llp(cur), _dp(joint),
                                           _dp(ms), _dp(push), _dp(state), _llp(count), _ip(word), _dp(meas), _dp(rows), _dp(frows),
                                           _dp(qrows), _ip(status)), "rollout_qp")
        return meas, rows, frows, qrows, status, state, count, word

    def start_feedback(self, nodes, t0, row, meas, params, start, cursor=None, map_id=None, goal_step=None, goal=None, err=None,
                       status=None):
        """Feedback hand-over (qtos_start_feedback, host form; the rule: feedback.start_feedback): the start vectors `start`
        (B x 24, qtos_handover's) corrected by the tracking error of the plans `nodes` at their hand-over rows `row`, from the
        measured rows `meas` -- (B, rows, 18), or (B, rows, 19) with params' quaternion flag, rows = params.n_rows (table mode) or
        params.capacity (a ring, addressed with `cursor` as track() addresses it).  params: a QtosFeedback (feedback_params()).
        map_id (B): the handle's heightfield of every window (None: map 0).  goal_step and goal (B x 3) go together: goal[:, 0:2]
        = start[:, 0:2] + goal_step[:, 0:2] of the corrected start.  err (B x 18) and status (B) are the arrays as they stand
        (None: zeros): a window without a measurement keeps its entries.  Returns new arrays (start, goal or None, err, status)."""
        self._need("qtos_start_feedback", "feedback hand-over")
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        row, mid = _bcast(row, B, np.int32), _bcast(map_id, B, np.int32)
        meas = _meas(meas, B, _rows(params), params.flags & FEEDBACK_QUAT)
        cur = _segment(params, B, cursor)[1]
        _goal_pair(goal_step, goal)
        gs, gl = _mat(goal_step, (B, 3)), _mat(goal, (B, 3), copy=True)
        start = _mat(start, (B, START_DOUBLES), copy=True)
        err = np.zeros((B, 18)) if err is None else _mat(err, (B, 18), copy=True)
        status = np.zeros(B, np.int32) if status is None else np.array(status, np.int32).reshape(B)
        self._chk(self.lib.qtos_start_feedback(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(row),
                                               _llp(cur), _dp(meas), _ip(mid), _dp(start), _dp(gs), _dp(gl), _dp(err), _ip(status)),
                  "start_feedback")
        return start, gl, err, status

    def plan_check(self, nodes, t0, params, map_id=None, first_row=None, n_rows=None, cursor=None, rows=True, summary=None,
                   stream=None):
        """What every plan in `nodes` violates between its knots (qtos_plan_check; the rule: plan_check.py).  params: a
        QtosPlanCheck (check_params()).  Returns (rows, summary): rows [B, params.n_rows, 27] (rows=True; an array: written into a
        copy of it, rows behind a window's count stay; False / None: no table) and summary [B, 5] records of plan_check.SUMMARY
        (summary=None with a table: computed as well; an array: with params' accumulate flag merged with it; False: none).
        first_row, n_rows: an int or B ints; cursor: B ints, the summary's rows count from it.  numpy arrays go through the host
        form.  torch tensors on the device (nodes, t0 and whichever of the others are given; rows / summary: tensors to write
        into, summary as B x 5 x 3 float64 words or None) go through the device form on `stream` (a torch stream; None: the
        current one) and come back as they are, without a synchronisation."""
        self._need("qtos_plan_check", "plan-check kernel")
        from . import plan_check as pc
        if hasattr(nodes, "data_ptr"):
            import torch
            st = torch.cuda.current_stream(nodes.device) if stream is None else stream
            B = nodes.reshape(-1, self.n).shape[0]
            p = ptr_given
            self._chk(self.lib.qtos_plan_check_device(self.h, B, C.byref(params), p(nodes), p(t0), p(map_id), p(first_row),
                                                      p(n_rows), p(cursor), p(rows), p(summary), C.c_void_p(st.cuda_stream)),
                      "plan_check_device")
            return (rows if p(rows) else None), (summary if p(summary) else None)
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        mid, first, per = _bcast(map_id, B, np.int32), _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        cur = _bcast(cursor, B, np.int64)
        rows = _table(rows, (B, int(params.n_rows), CHECK_COLS), reshape=True)
        summary = _summary(summary, rows, pc, B, CHECK_FAMILIES)
        self._chk(self.lib.qtos_plan_check(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(mid), _ip(first), _ip(per), _llp(cur),
                                           _dp(rows), _vp(summary)), "plan_check")
        return rows, summary

    def force_fit(self, nodes, t0, params, map_id=None, first_row=None, n_rows=None, cursor=None, joint=None, mass_scale=None,
                  rows=True, status=None, summary=None, stream=None):
        """The contact forces of every row of the plans in `nodes` fitted to the planned motion (qtos_force_fit; the rule:
        force_fit.py).  params: a QtosForceFit (fit_params()).  Returns (rows, status, summary): rows [B, R, 32] and status [B, R]
        int32, R = params.n_rows (table mode) or params.capacity (ring mode: `rows`, `status` and `cursor` are the rings as they
        stand) -- rows=True: new arrays; an array: written into a copy of it, rows behind a window's count stay; False / None: no
        table -- and summary [B, 4] records of force_fit.SUMMARY (summary=None with a table: computed as well; an array: with
        params' accumulate flag merged with it; False: none).  joint: [B, R, 37] joint rows in the same addressing (None: columns
        20 .. 31 are not touched); mass_scale: a number or B; first_row, n_rows: an int or B ints.  numpy arrays go through the host
        form.  torch tensors on the device (nodes, t0 and whichever of the others are given; rows, status, summary: tensors to
        write into, summary as B x 4 x 3 float64 words, or None) go through the device form on `stream` (a torch stream; None: the
        current one) and come back as they are, without a synchronisation."""
        self._need("qtos_force_fit", "force-fit kernel")
        from . import force_fit as ff
        if hasattr(nodes, "data_ptr"):
            import torch
            st = torch.cuda.current_stream(nodes.device) if stream is None else stream
            B = nodes.reshape(-1, self.n).shape[0]
            p = ptr_given
            self._chk(self.lib.qtos_force_fit_device(self.h, B, C.byref(params), p(nodes), p(t0), p(map_id), p(first_row),
                                                     p(n_rows), p(cursor), p(joint), p(mass_scale), p(rows), p(status),
                                                     p(summary), C.c_void_p(st.cuda_stream)), "force_fit_device")
            return (rows if p(rows) else None), (status if p(status) else None), (summary if p(summary) else None)
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        mid, first, per = _bcast(map_id, B, np.int32), _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        keep = not (rows is False or rows is None)
        nr, cur = _segment(params, B, cursor, *((rows, status) if keep and params.capacity > 0 else ()))
        nr = max(nr, 0)
        joint = None if joint is None else np.ascontiguousarray(joint, np.float64)
        if joint is not None and joint.shape != (B, nr, CSV_COLS):
            raise ValueError("joint is (B, %d, %d)" % (nr, CSV_COLS))
        ms = _bcast(mass_scale, B)
        rows = _table(rows, (B, nr, FIT_COLS))
        if rows is None:
            status = None
        else:
            status = np.zeros((B, nr), np.int32) if status is None else np.array(status, np.int32)
            if rows.shape != (B, nr, FIT_COLS) or status.shape != (B, nr):
                raise ValueError("rows is (B, %d, %d) and status (B, %d)" % (nr, FIT_COLS, nr))
        summary = _summary(summary, rows, ff, B, FIT_FAMILIES)
        self._chk(self.lib.qtos_force_fit(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(mid), _ip(first), _ip(per), _llp(cur),
                                          _dp(joint), _dp(ms), _dp(rows), _ip(status), _vp(summary)), "force_fit")
        return rows, status, summary

    def force_qp(self, nodes, t0, params, map_id=None, first_row=None, n_rows=None, cursor=None, joint=None, mass_scale=None,
                 rows=True, qrows=True, status=None, summary=None, stream=None):
        """The force fit inside the friction pyramid (qtos_force_qp; the rule: force_qp.py).  params: a QtosForceQp (qp_params()).
        The arguments are force_fit's; returns (rows, qrows, status, summary): rows [B, R, 32], qrows [B, R, 8] the solve's table
        (True: a new array with rows; an array: written into a copy; False / None: none) and summary [B, 4] records of the families
        res_ang, res_lin, change, limited.  torch tensors on the device go through the device form on `stream`."""
        self._need("qtos_force_qp", "force-QP kernel")
        from . import force_qp as fq
        if hasattr(nodes, "data_ptr"):
            import torch
            st = torch.cuda.current_stream(nodes.device) if stream is None else stream
            B = nodes.reshape(-1, self.n).shape[0]
            p = ptr_given
            self._chk(self.lib.qtos_force_qp_device(self.h, B, C.byref(params), p(nodes), p(t0), p(map_id), p(first_row), p(n_rows),
                                                    p(cursor), p(joint), p(mass_scale), p(rows), p(qrows), p(status), p(summary),
                                                    C.c_void_p(st.cuda_stream)), "force_qp_device")
            return (rows if p(rows) else None), (qrows if p(qrows) else None), (status if p(status) else None), (summary if p(summary) else None)
        nodes, B = self._nodes(nodes)
        t0 = _bcast(t0, B)
        mid, first, per = _bcast(map_id, B, np.int32), _bcast(first_row, B, np.int32), _bcast(n_rows, B, np.int32)
        keep = not (rows is False or rows is None)
        nr, cur = _segment(params, B, cursor, *((rows, status) if keep and params.capacity > 0 else ()))
        nr = max(nr, 0)
        joint = None if joint is None else np.ascontiguousarray(joint, np.float64)
        if joint is not None and joint.shape != (B, nr, CSV_COLS):
            raise ValueError("joint is (B, %d, %d)" % (nr, CSV_COLS))
        ms = _bcast(mass_scale, B)
        rows = _table(rows, (B, nr, FIT_COLS))
        if rows is None:
            status = qrows = None
        else:
            status = np.zeros((B, nr), np.int32) if status is None else np.array(status, np.int32)
            qrows = _table(qrows, (B, nr, QP_COLS))
            if rows.shape != (B, nr, FIT_COLS) or status.shape != (B, nr) or (qrows is not None and qrows.shape != (B, nr, QP_COLS)):
                raise ValueError("rows is (B, %d, %d), qrows (B, %d, %d) and status (B, %d)" % (nr, FIT_COLS, nr, QP_COLS, nr))
        summary = _summary(summary, rows, fq, B, FIT_FAMILIES)
        self._chk(self.lib.qtos_force_qp(self.h, B, C.byref(params), _dp(nodes), _dp(t0), _ip(mid), _ip(first), _ip(per), _llp(cur),
                                         _dp(joint), _dp(ms), _dp(rows), _dp(qrows), _ip(status), _vp(summary)), "force_qp")
        return rows, qrows, status, summary

    def path_goal(self, table, clock, params, path_id=None, map_yx=None, map_id=None, offset=None, start=None, done=None):
        """Goals of the windows' next plans from their global paths (qtos_path_goal, host form; the rule:
        global_planner.path_goal).  table: global_planner.path_table; clock [B]; params: a QtosPathGoal (path_goal_params; the
        sizes of the table and the grids are filled in here); path_id [B] (None: window b follows path b); map_yx n_maps x rows x
        cols or rows x cols (None: every height 0) with map_id [B] (None: map 0); offset [B] (None: 0); start [B, 24] (None where
        nothing reads it); done [B] (None: no done bits are kept).  Returns new arrays (goal [B, 3], done [B] int32 or None,
        clock [B])."""
        self._need("qtos_path_goal", "path-goal kernel")
        clock = np.array(clock, np.float64).reshape(-1)
        B = len(clock)
        g = params.copy()
        knots = np.ascontiguousarray(table["knots"], np.float64)
        coef = np.ascontiguousarray(table["coef"], np.float64)
        npc = np.ascontiguousarray(table["n_pieces"], np.int32)
        rg = None if table.get("robot_goal") is None else np.ascontiguousarray(table["robot_goal"], np.float64)
        g.n_paths, g.max_pieces = coef.shape[0], coef.shape[3]
        if knots.shape != (g.n_paths, g.max_pieces + 1) or coef.shape[1:3] != (2, 4) or npc.shape != (g.n_paths,):
            raise ValueError("not a path table: knots [n_paths, max_pieces + 1], coef [n_paths, 2, 4, max_pieces], n_pieces [n_paths]")
        grids = None
        if map_yx is not None:
            grids = _maps(map_yx)
            g.n_maps, g.rows, g.cols = grids.shape
        pid, mid, off = _vec(path_id, B), _vec(map_id, B), _bcast(offset, B)
        st = _mat(start, (B, START_DOUBLES))
        dn = None if done is None else np.array(done, np.int32).reshape(B)
        goal = np.empty((B, 3))
        self._chk(self.lib.qtos_path_goal(self.h, B, C.byref(g), _dp(knots), _dp(coef), _ip(npc), _dp(rg), _ip(pid), _dp(grids), _ip(mid),
                                          _dp(clock), _dp(off), _dp(st), _dp(goal), _ip(dn)), "path_goal")
        return goal, dn, clock

    def path_plan(self, bool_map, start, robot_goal, params, map_id=None, done=None, cells=True):
        """The windows' global paths, planned on the device (qtos_path_plan, host form; the rule: global_planner.path_plan).
        bool_map n_maps x rows x cols or rows x cols with map_id [B] (None: map 0); start [B, 24] or [B, 2] (x, y); robot_goal
        [B, 3]; params: a QtosPathPlan (path_plan_params; the maps' sizes are filled in here); done [B] (None: no done bits);
        cells False: the paths' cells are not kept.  Returns the dict of global_planner.path_plan: the path table (knots, coef,
        n_pieces, robot_goal) plus cells (or None), n_cells, status, and done where it was given."""
        self._need("qtos_path_plan", "path-plan kernel")
        g = params.copy()
        maps = _maps(bool_map)
        g.n_maps, g.rows, g.cols = maps.shape
        rg = np.ascontiguousarray(robot_goal, np.float64)
        B = rg.shape[0]
        rg = rg.reshape(B, 3)
        st = np.asarray(start, np.float64).reshape(B, -1)
        if st.shape[1] != START_DOUBLES:
            st = np.concatenate([st[:, 0:2], np.zeros((B, START_DOUBLES - 2))], axis=1)
        st = np.ascontiguousarray(st)
        mid = _vec(map_id, B)
        dn = None if done is None else np.array(done, np.int32).reshape(B)
        mp, mc = max(g.max_pieces, 1), max(g.max_cells, 1)     # (sizes of the arrays only: the library checks the values)
        knots, coef, npc = np.zeros((B, mp + 1)), np.zeros((B, 2, 4, mp)), np.zeros(B, np.int32)
        cl = np.zeros((B, mc, 2), np.int32) if cells else None
        ncl, status = np.zeros(B, np.int32), np.zeros(B, np.int32)
        self._chk(self.lib.qtos_path_plan(self.h, B, C.byref(g), _dp(maps), _ip(mid), _dp(st), _dp(rg), _dp(knots), _dp(coef), _ip(npc),
                                          _ip(cl), _ip(ncl), _ip(status), _ip(dn)), "path_plan")
        out = dict(knots=knots, coef=coef, n_pieces=npc, robot_goal=rg.copy(), cells=cl, n_cells=ncl, status=status)
        if dn is not None:
            out["done"] = dn
        return out

    def probe(self, map_yx, params=None, capacity=None):
        """The probe patches of the maps as solver problems (qtos_probe, host form; the rule: feasibility.probe_table).  map_yx
        n_maps x rows x cols or rows x cols; params: a QtosProbe (probe_params; the maps' sizes are filled in here); capacity: room
        for that many problems (None: a first call with capacity 0 reads their number, a second one fills arrays of that size).
        Returns the dict of feasibility.probe_table -- offsets, slot, patch, start, goal, map_id, the last four with
        min(N, capacity) rows."""
        self._need("qtos_probe", "probe kernels")
        maps = _maps(map_yx)
        g = (params or probe_params()).copy()
        g.n_maps, g.rows, g.cols = maps.shape
        offsets = np.zeros(g.n_maps + 1, np.int32)
        slot = np.zeros((g.n_maps, g.rows, max(g.cols // 2 - 1, 0)), np.int32)

        def call(cap):
            out = dict(patch=np.zeros((cap, 3), np.int32), start=np.zeros((cap, START_DOUBLES)), goal=np.zeros((cap, 3)),
                       map_id=np.zeros(cap, np.int32))
            self._chk(self.lib.qtos_probe(self.h, C.byref(g), _dp(maps), cap, _ip(offsets), _ip(slot), _ip(out["patch"]), _dp(out["start"]),
                                          _dp(out["goal"]), _ip(out["map_id"])), "probe")
            return out
        out = call(0 if capacity is None else int(capacity))
        if capacity is None and offsets[-1] > 0:
            out = call(int(offsets[-1]))
        n = min(int(offsets[-1]), len(out["patch"]))
        return dict(offsets=offsets, slot=slot, **{k: v[:n] for k, v in out.items()})

    def probe_stamp(self, shape, offsets, slot, patch, status, params=None):
        """Exit statuses -> boolean maps (qtos_probe_stamp, host form; the rule: feasibility.stamp_table).  shape (rows, cols) or
        (n_maps, rows, cols); offsets, slot, patch as probe() returned them; status [offsets[-1]].  Returns n_maps x rows x cols
        doubles of 0.0 / 1.0."""
        self._need("qtos_probe_stamp", "probe kernels")
        offsets = np.ascontiguousarray(offsets, np.int32)
        g = (params or probe_params()).copy()
        g.n_maps, (g.rows, g.cols) = len(offsets) - 1, tuple(shape)[-2:]
        slot = np.ascontiguousarray(slot, np.int32)
        patch = None if patch is None else np.ascontiguousarray(patch, np.int32).reshape(-1, 3)     # (not read by the library)
        status = _vec(status, -1)
        N = int(offsets[-1])
        if slot.size != g.n_maps * g.rows * max(g.cols // 2 - 1, 0) or len(status) < N or (patch is not None and len(patch) < N):
            raise ValueError("slot is n_maps x rows x (cols // 2 - 1); patch (or None) and status hold offsets[-1] entries")
        out = np.zeros((g.n_maps, g.rows, g.cols))
        self._chk(self.lib.qtos_probe_stamp(self.h, C.byref(g), _ip(offsets), _ip(slot), _ip(patch), _ip(status), _dp(out)), "probe_stamp")
        return out

    def terrain_env(self, base_yx, seed, draws=None, base_id=None, params=None, map_yx=None, height_xy=None):
        """The randomised terrains of the maps (qtos_terrain_env, host form; the rule: heightfield.random_env_table).  base_yx
        n_base x rows x cols or rows x cols; seed [n_maps] (0 .. 2**64 - 1); draws [n_maps] outputs already consumed (None: 0);
        base_id [n_maps] or None (map m reads base m); params: a QtosTerrainEnv (terrain_env_params; the sizes are filled in
        here); map_yx, height_xy: arrays the call writes into (None: zeros) -- a map with a non-zero status keeps what they
        hold.  Returns the dict of random_env_table: map_yx, height_xy, draws, status."""
        self._need("qtos_terrain_env", "terrain-env kernel")
        base = _maps(base_yx)
        seed = np.ascontiguousarray([int(v) for v in np.ravel(seed)], np.uint64)
        g = (params or terrain_env_params()).copy()
        g.n_maps, (g.n_base, g.rows, g.cols) = len(seed), base.shape
        draws = np.zeros(g.n_maps, np.int32) if draws is None else np.array(draws, np.int32).reshape(g.n_maps)
        bid = _vec(base_id, g.n_maps)
        out_m = np.zeros((g.n_maps, g.rows, g.cols)) if map_yx is None else map_yx
        out_h = np.zeros((g.n_maps, g.cols, g.rows)) if height_xy is None else height_xy
        for a in (out_m, out_h):
            if a.dtype != np.float64 or not a.flags.c_contiguous or a.size != g.n_maps * g.rows * g.cols:
                raise ValueError("map_yx and height_xy are contiguous float64 arrays of n_maps x rows x cols values")
        status = np.zeros(g.n_maps, np.int32)
        self._chk(self.lib.qtos_terrain_env(self.h, C.byref(g), _dp(base), _ip(bid), seed.ctypes.data_as(C.POINTER(C.c_uint64)), _ip(draws),
                                            _dp(out_m), _dp(out_h), _ip(status)), "terrain_env")
        return dict(map_yx=out_m, height_xy=out_h, draws=draws, status=status)

    def set_heightfields_device(self, height_xy, cell, x0=-1.0, y0=-1.0, stream=None):
        """set_heightfields from a tensor on the planner's device (n_maps x nx x ny or nx x ny, float64; e.g. height_xy of
        qtos_terrain_env_device): copied device-to-device on `stream` (a torch stream; None: the current one), no host trip.  A
        tensor that is not contiguous -- a stack of `heightfield.towr_map` results is not: they are transposes -- is made so
        on that stream first.  The library orders the copy behind the handle's last call and in front of whatever the handle
        runs next -- `plan`, `probe`, ... on its own stream, a device-form solve on any stream --, so no synchronisation is
        needed round this call; RuntimeError (-5) while a call is open."""
        import torch
        if not self.has("qtos_set_heightfields_device"):
            raise RuntimeError("this build of the planner library has no qtos_set_heightfields_device")
        t = height_xy[None] if height_xy.dim() == 2 else height_xy
        if not t.is_cuda or t.device.index != self.device or t.dtype != torch.float64 or t.dim() != 3:
            raise ValueError("height_xy is a float64 tensor n_maps x nx x ny on the planner's device")
        stream = torch.cuda.current_stream(t.device) if stream is None else stream
        with torch.cuda.stream(stream):
            t = t.contiguous()
            self._chk(self.lib.qtos_set_heightfields_device(self.h, t.shape[0], t.data_ptr(), t.shape[1], t.shape[2], cell, x0, y0,
                                                            C.c_void_p(stream.cuda_stream)), "set_heightfields_device")

    # ---- optional: nominal-plan table for the starting point of cold solves ----
    def set_init_table(self, dx=None, dy=None, nodes=None):
        """Install (or, without arguments, remove) a table of nominal plans: nodes[j][i] = the plan from the
        rest start at the origin to the goal (dx[i], dy[j])."""
        if dx is None:
            self._chk(self.lib.qtos_set_init_table(self.h, 0, None, 0, None, None), "set_init_table")
            self.init_table = None
            return
        dx = np.ascontiguousarray(dx, np.float64)
        dy = np.ascontiguousarray(dy, np.float64)
        nodes = _mat(nodes, (len(dy), len(dx), self.n))
        self._chk(self.lib.qtos_set_init_table(self.h, len(dx), _dp(dx), len(dy), _dp(dy), _dp(nodes)), "set_init_table")
        self.init_table = (dx, dy, nodes)

    def build_init_table(self, dx=None, dy=None, z=0.24):
        """Solve the nominal problems (rest start at the origin, nominal stance, current heightfields,
        straight-line guess) on a grid of goal displacements and install them as the table.  Default
        grid: 0.1 .. 0.16 m per second of horizon ahead in five steps, -0.1 .. 0.1 m sideways in three."""
        from . import workloads
        T = self.dims.duration
        dx = np.asarray(dx if dx is not None else np.linspace(0.03, 0.15, 5) * T, np.float64)
        dy = np.asarray(dy if dy is not None else [-0.1, 0.0, 0.1], np.float64)
        self.set_init_table()
        start = np.repeat(workloads.rest_start(0.0, 0.0, z)[None], len(dx) * len(dy), 0)
        goal = np.array([[x, y, z] for y in dy for x in dx])
        nodes = np.empty((len(goal), self.n))
        for i in range(0, len(goal), self.max_batch):
            sl = slice(i, i + self.max_batch)
            nodes[sl], status, _, _ = self.plan(start[sl], goal[sl])
            if (status != 0).any():
                raise RuntimeError("a nominal plan of the table did not converge")
        self.set_init_table(dx, dy, nodes)
        return dx, dy

    def initial_guess(self, start, goal, map_id=None):
        """The starting point a solve without `warm` uses for these problems (tests: the oracle is started
        from the same point)."""
        start, goal, mid = _mat(start, (-1, START_DOUBLES)), _mat(goal, (-1, 3)), _vec(map_id, -1)
        out = np.empty((start.shape[0], self.n))
        self._chk(self.lib.qtos_debug_initial_guess(self.h, start.shape[0], _dp(start), _dp(goal), _ip(mid), _dp(out)), "initial_guess")
        return out

    def kkt_kernel(self):
        """Name of the factor + solve kernel the planner selected (the one rocprofv3 lists), e.g. 'k_kkt3<96, 1>'."""
        buf = C.create_string_buffer(64)
        self._chk(min(self.lib.qtos_kkt_kernel(self.h, buf, 64), 0), "kkt_kernel")
        return buf.value.decode()

    def timing(self):
        k, t = C.c_double(), C.c_double()
        nl, it = C.c_int(), C.c_int()
        self._chk(self.lib.qtos_last_timing(self.h, C.byref(k), C.byref(nl), C.byref(t), C.byref(it)), "last_timing")
        out = dict(kkt_seconds=k.value, kkt_launches=nl.value, total_seconds=t.value, iterations=it.value)
        if self.has("qtos_last_timing_chord"):
            c, nc = C.c_double(), C.c_int()
            self._chk(self.lib.qtos_last_timing_chord(self.h, C.byref(c), C.byref(nc)), "last_timing_chord")
            out.update(chord_seconds=c.value, chord_launches=nc.value)
        return out

    def totals(self, reset=False):
        """(problems returned with status 0, Newton iterations) over all plan calls of this handle since the last reset."""
        c, n = C.c_longlong(), C.c_longlong()
        self._chk(self.lib.qtos_plan_totals(self.h, C.byref(c), C.byref(n), int(bool(reset))), "plan_totals")
        return c.value, n.value

    # ---- introspection (parity tests) ----
    def debug_eval(self, start, goal, nodes, map_id=None, jac=True):
        start, goal, mid = _mat(start, (-1, START_DOUBLES)), _mat(goal, (-1, 3)), _vec(map_id, -1)
        nodes = self._nodes(nodes)[0]
        B = start.shape[0]
        g = np.empty((B, self.m))
        J = np.empty((B, self.m, self.n)) if jac else None
        self._chk(self.lib.qtos_debug_eval(self.h, B, _dp(start), _dp(goal), _ip(mid), _dp(nodes), _dp(g), _dp(J)), "debug_eval")
        return g, J

    def debug_newton(self, start, goal, nodes, sig, w, map_id=None):
        start, goal, mid = _mat(start, (-1, START_DOUBLES)), _mat(goal, (-1, 3)), _vec(map_id, -1)
        nodes = self._nodes(nodes)[0]
        B = start.shape[0]
        sig, w = _mat(sig, (B, self.m)), _mat(w, (B, self.m))
        dx = np.empty((B, self.n))
        self._chk(self.lib.qtos_debug_newton(self.h, B, _dp(start), _dp(goal), _ip(mid), _dp(nodes), _dp(sig), _dp(w), _dp(dx)), "debug_newton")
        return dx

    def debug_chord(self, B):
        """dx of the system of the preceding debug_newton call, solved again by k_chord with the stored factorisation."""
        dx = np.empty((B, self.n))
        self._chk(self.lib.qtos_debug_chord(self.h, B, _dp(dx)), "debug_chord")
        return dx

    def project(self, nodes):
        """What given nodes become when a solve starts from them (reduce_base: their projection onto the space of the base's
        B-spline coefficients; otherwise a copy)."""
        nodes, B = self._nodes(nodes)
        out = np.empty_like(nodes)
        self._chk(self.lib.qtos_project_nodes(self.h, B, _dp(nodes), _dp(out)), "project_nodes")
        return out

    def debug_residual(self, B, refine=False):
        """(dx, max |b - K x| / max |b| per problem) of the system of the preceding debug_newton call; refine: after one
        step of iterative refinement through the stored factorisation."""
        dx = np.empty((B, self.n))
        res = np.empty(B)
        self._chk(self.lib.qtos_debug_residual(self.h, B, int(bool(refine)), _dp(dx), _dp(res)), "debug_residual")
        return dx, res

    def structure(self):
        rk = np.empty(self.m, np.int32)
        vf = np.empty(self.n, np.int32)
        order = np.empty(self.dims.n_stages * self.dims.pivots, np.int32)    # by position; -1 = a dummy pivot (short stage)
        self.lib.qtos_debug_structure(self.h, _ip(rk), _ip(vf), _ip(order))
        return rk, vf, order

    def factor(self, b):
        """(panels [n_stages, front + 1, 16], pivot slots [n_stages, 16]) of problem b's last KKT solve."""
        d = self.dims
        pan = np.zeros((d.n_stages, d.front + 1, 16))
        ps = np.zeros((d.n_stages, 16), dtype=np.int32)
        self._chk(self.lib.qtos_debug_factor(self.h, b, _dp(pan), _ip(ps)), "qtos_debug_factor")
        # in memory column c of a V row sits at 4 (c & 3) + (c >> 2) (32 contiguous bytes per lane on the store)
        cols = np.array([4 * (c & 3) + (c >> 2) for c in range(16)])
        pan[:, 1:, :] = pan[:, 1:, :][:, :, cols]
        return pan, ps

    def trace(self, b):
        t = np.zeros((self.cfg.max_iter + 1, 4))
        rows = self.lib.qtos_debug_trace(self.h, b, _dp(t))
        return t[:max(rows, 0)]
