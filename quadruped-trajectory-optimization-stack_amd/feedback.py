"""Feedback hand-over: the rule of k_start_feedback (qtos_start_feedback*, include/qtos_planner.h) stated in numpy.

k_handover starts every new plan from the old plan's own hand-over row, as the reference's ``Combiner._state`` does: the reference
records ``robot_state`` in ``Global_Planner.update`` and never uses it.  This rule corrects that start vector by the tracking error
of the plan handed over from -- the measured pose of ``tracking.measured_pose`` against the plan's own row -- so that the next
plan starts where the robot is.  With every gain 0 it changes nothing, to the bit.

The number type is a parameter, as in tracking.py: dtype = np.longdouble is what the kernel is held to, np.float64 the same
formulas in the kernel's own precision.  The terrain heights are float64 look-ups in every dtype: the kernel's.
"""
import math

import numpy as np

from . import joints, tracking
from .joints import NEE
from .stitcher import ring_index

CORRECTED, CLIPPED, GIMBAL, FALLBACK, NO_MEASUREMENT = 1, 2, 4, 8, 32      # status bits of a window
SNAPPED = 64                                                                 # << f: foot f's z moved by more than snap_tol
FLAG_QUAT, FLAG_SNAP, FLAG_ZERO_FILTER = 1, 2, 4                             # QtosFeedback.flags: QTOS_FEEDBACK_*
TWO_PI = 6.283185307179586


class FeedbackParams(tracking.TrackParams):
    """What start_feedback reads: the leg data and ee_shift of tracking.TrackParams, the addressing of the measured rows, the
    latency, the gains, the clips and the range-of-motion box.  capi.QtosFeedback has the same field names and is taken as well.
    nominal and max_deviation default to PlannerConfig's."""

    def __init__(self, robot=joints.SOLO12, ee_shift=0.015, quaternion=False, hz=1000.0, first_row=0, n_rows=0, capacity=0, latency=0.0,
                 gain_pos=1.0, gain_ang=1.0, gain_foot=1.0, max_pos=0.05, max_ang=0.2, max_foot=0.05, nominal=None, max_deviation=None,
                 rom_tol=1e-6, snap_tol=0.02, snap=True, zero_filter=False):
        tracking.TrackParams.__init__(self, robot=robot, ee_shift=ee_shift, delay=0, quaternion=quaternion)
        if nominal is None or max_deviation is None:
            from .config import PlannerConfig
            cfg = PlannerConfig()
            nominal = cfg.nominal_stance if nominal is None else nominal
            max_deviation = cfg.max_deviation if max_deviation is None else max_deviation
        self.hz, self.first_row, self.n_rows, self.capacity = float(hz), int(first_row), int(n_rows), int(capacity)
        self.latency = float(latency)
        self.gain_pos, self.gain_ang, self.gain_foot = float(gain_pos), float(gain_ang), float(gain_foot)
        self.max_pos, self.max_ang, self.max_foot = float(max_pos), float(max_ang), float(max_foot)
        self.nominal = np.array(nominal, np.float64).reshape(NEE, 3)
        self.max_deviation = np.array(max_deviation, np.float64).reshape(3)
        self.rom_tol, self.snap_tol = float(rom_tol), float(snap_tol)
        self.flags = (FLAG_QUAT if quaternion else 0) | (FLAG_SNAP if snap else 0) | (FLAG_ZERO_FILTER if zero_filter else 0)


def terrain_lookup(height_xy=None, cell=0.1, x0=-1.0, y0=-1.0, mode=1):
    """The ``height`` argument of start_feedback for heightfields as the planner holds them (n_maps x nx x ny or nx x ny; None:
    flat ground): height(map_id, x, y) through heightfield.height_at, the lookup the oracle's qo_terrain_height is tested
    against, in the planner's terrain_mode (0 bilinear, 1 nearest cell).  A map id outside the maps reads the nearest one."""
    if height_xy is None:
        return lambda map_id, x, y: 0.0
    from . import heightfield
    maps = np.asarray(height_xy, np.float64)
    maps = maps[None] if maps.ndim == 2 else maps

    def height(map_id, x, y):
        m = min(max(int(map_id), 0), len(maps) - 1)
        return float(heightfield.height_at(maps[m], cell, float(x), float(y), x0, y0, mode))
    return height


def lag_rows(params):
    """round(latency * hz), halves away from zero: the C library's round."""
    hz = float(params.hz) if float(params.hz) > 0 else 1000.0
    return int(math.floor(float(params.latency) * hz + 0.5))


def measured_row(row, params):
    """(k, j): the plan row the measurement belongs to, clamp(row - lat, first_row, first_row + row - 1), and its place k -
    first_row in the segment; None where the window has no measurement: row <= 0, or a place the table (n_rows) or the ring
    (capacity) does not hold."""
    r, first = int(row), int(params.first_row)
    if r <= 0:
        return None
    k = min(max(r - lag_rows(params), first), first + r - 1)
    j = k - first
    held = int(params.capacity) if int(params.capacity) > 0 else int(params.n_rows)
    return None if j >= held else (k, j)


def wrap_yaw(d, dtype):
    """The IEEE remainder of d with 2 pi (the float64 nearest 2 pi in every dtype): math.remainder, C's remainder."""
    if dtype is np.float64:
        return np.float64(math.remainder(float(d), TWO_PI))
    tp = dtype(TWO_PI)
    return d - tp * np.rint(d / tp)


def start_feedback(L, x, t0, row, meas, params, start, height=None, map_id=0, goal_step=None, cursor=0, dtype=np.longdouble):
    """One window.  L, x, t0: the plan handed over from (oracle.splines.layout, its nodes, its clock); row: the hand-over row;
    meas: the window's measured rows [n_rows | capacity, 18 | 19], table or ring with `cursor` as tracking.track_ring addresses
    it; start [24]: k_handover's start vector; height: None (flat) or height(map_id, x, y) (terrain_lookup).  Returns (start [24]
    in dtype, goal_xy [2] or None, err [18], status):

      measurement  plan row k of measured_row; none: status NO_MEASUREMENT, start as it came, goal None, err zeros
      e            measured_pose - the plan's columns 1 .. 18 of row k, the yaw through wrap_yaw, clipped to +- max_pos (CoM), +-
                   max_ang (Euler), +- max_foot (feet): CLIPPED where a clip acted, GIMBAL from measured_pose
      correction   start[0:3] += gain_pos e[0:3], start[3:6] += gain_ang e[3:6], feet += gain_foot e[6:18]; a gain of 0 adds
                   nothing, and with every gain 0 the rule ends here: the start as it came, to the bit, the status CLIPPED and
                   GIMBAL only, goal_xy from that start.  With the snap every foot's z is then height(map_id, x, y) at its
                   corrected x, y (SNAPPED << f: that is more than snap_tol from the corrected z)
      guard        d_f = R(corrected Euler)^T (foot_f - com) - nominal[f]; unless every |d_f[i]| <= max_deviation[i] + rom_tol:
                   FALLBACK, the start as it came
      CORRECTED    a measurement, no fallback, a gain that is not 0.  Zero filter (|v| < 1e-4 -> 0) on the 24 numbers of a window
                   that did not fall back.  goal_xy = start[0:2] + goal_step[0:2] of the start that is returned."""
    s_in = np.asarray(start).astype(dtype).reshape(24)
    err = np.zeros(18, dtype)
    at = measured_row(row, params)
    if at is None:
        return s_in.copy(), None, err, NO_MEASUREMENT
    k, j = at
    cap = int(params.capacity)
    m_row = meas[ring_index(cursor, j + 1, cap)[j]] if cap > 0 else meas[j]        # (only this row is read)
    hz = float(params.hz) if float(params.hz) > 0 else 1000.0
    pose, gimbal = tracking.measured_pose(m_row, params, dtype, with_status=True)
    plan = tracking.plan_positions(L, x, t0, hz, k, 1, dtype)[0, 1:19]
    status = int(gimbal) & GIMBAL
    e = pose - plan
    e[5] = wrap_yaw(e[5], dtype)
    clip = np.array([params.max_pos] * 3 + [params.max_ang] * 3 + [params.max_foot] * 12, np.float64).astype(dtype)
    for i in range(18):
        if e[i] < -clip[i]:
            e[i], status = -clip[i], status | CLIPPED
        elif e[i] > clip[i]:
            e[i], status = clip[i], status | CLIPPED
    err[:] = e
    gains = (float(params.gain_pos), float(params.gain_ang), float(params.gain_foot))
    step = None if goal_step is None else np.asarray(goal_step).astype(dtype).reshape(-1)[0:2]
    if not any(g != 0 for g in gains):
        return s_in.copy(), None if step is None else s_in[0:2] + step, err, status
    c = s_in.copy()
    for lo, hi, g in ((0, 3, params.gain_pos), (3, 6, params.gain_ang), (6, 18, params.gain_foot)):
        if float(g) != 0:
            c[lo:hi] = s_in[lo:hi] + dtype(np.float64(g)) * e[lo:hi]
    if int(params.flags) & FLAG_SNAP:
        h = height if height is not None else terrain_lookup()
        for f in range(NEE):
            z = dtype(np.float64(h(map_id, np.float64(c[6 + 3 * f]), np.float64(c[7 + 3 * f]))))
            if abs(z - c[8 + 3 * f]) > dtype(np.float64(params.snap_tol)):
                status |= SNAPPED << f
            c[8 + 3 * f] = z
    R = joints.rotation(c[3:6], dtype)
    nominal = np.array(params.nominal, np.float64).reshape(NEE, 3).astype(dtype)
    bound = np.array(params.max_deviation, np.float64).reshape(3).astype(dtype) + dtype(np.float64(params.rom_tol))
    inside = True
    for f in range(NEE):
        v = c[6 + 3 * f:9 + 3 * f] - c[0:3]
        for i in range(3):
            d = ((R[0, i] * v[0] + R[1, i] * v[1]) + R[2, i] * v[2]) - nominal[f, i]
            inside = inside and bool(abs(d) <= bound[i])
    if not inside:
        out, status = s_in.copy(), status | FALLBACK
    else:
        out, status = c, status | CORRECTED
        if int(params.flags) & FLAG_ZERO_FILTER:
            out[np.abs(out) < dtype(1e-4)] = 0
    return out, None if step is None else out[0:2] + step, err, status


def start_feedback_batch(L, nodes, t0, row, meas, params, start, height=None, map_id=None, goal_step=None, cursor=None,
                         dtype=np.longdouble):
    """start_feedback for B windows: (start [B, 24], goal_xy [B, 2] (NaN rows where a window has no measurement) or None, err [B,
    18], status [B] int32)."""
    B = len(start)
    out, err, st = np.zeros((B, 24), dtype), np.zeros((B, 18), dtype), np.zeros(B, np.int32)
    goal = None if goal_step is None else np.full((B, 2), np.nan, dtype)
    for b in range(B):
        r = start_feedback(L, nodes[b], np.asarray(t0)[b], np.asarray(row)[b], meas[b], params, start[b], height,
                           0 if map_id is None else int(np.asarray(map_id)[b]), None if goal_step is None else goal_step[b],
                           0 if cursor is None else int(np.asarray(cursor)[b]), dtype)
        out[b], err[b], st[b] = r[0], r[2], r[3]
        if goal is not None and r[1] is not None:
            goal[b] = r[1]
    return out, goal, err, st
