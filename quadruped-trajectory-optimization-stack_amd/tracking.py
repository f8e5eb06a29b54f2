"""Measured states and tracking errors of a plan: the rule of k_track (qtos_track*, include/qtos_planner.h) stated in numpy.

What the reference does with the measured state once per 1 kHz tick (scripts/run.py:244-273, QTOS/tracking.py,
QTOS/robot/robot.py ``traj_vec``):

  * the base pose and the joint state become the 18-vector ``traj_vec``: CoM, Euler angles, four feet in the world
  * ``Tracking._update`` compares it with the CSV row just commanded: five Euclidean errors and two running totals
  * ``global_COM_xyz[0] >= goal[0]`` ends the run

The only thing the reference's simulator adds to ``traj_vec`` is forward kinematics, and the SOLO12 leg's closed form is
``joints.leg_fk``.  The number type is a parameter, as in joints.py and oracle/splines.py: dtype = np.longdouble is what the
kernel is held to, np.float64 the same formulas in the kernel's own precision.  The running totals are float64 additions in
program order in every dtype: they are the reference's Python floats.
"""
import numpy as np

from . import joints
from .joints import NEE
from .stitcher import ring_index

TRACK_COLS = 26
RECORDED, REACHED, GIMBAL = 1, 2, 4        # status bits of a row
FLAG_QUAT, FLAG_CLEAN_DELAY = 1, 2         # QtosTrack.flags: QTOS_TRACK_QUAT, QTOS_TRACK_CLEAN_DELAY
RULES = ("reference", "clean")


class TrackParams(joints.JointParams):
    """What track_rows reads: the leg data and ee_shift of joints.JointParams, the delay and the flags.  capi.QtosTrack has
    the same field names and is taken as well."""

    def __init__(self, robot=joints.SOLO12, ee_shift=0.015, delay=500, rule="reference", quaternion=False):
        joints.JointParams.__init__(self, robot=robot, ee_shift=ee_shift)
        if rule not in RULES:
            raise ValueError("rule is 'reference' or 'clean'")
        self.delay = int(delay)
        self.flags = (FLAG_QUAT if quaternion else 0) | (FLAG_CLEAN_DELAY if rule == "clean" else 0)


def rule_of(params):
    return "clean" if int(params.flags) & FLAG_CLEAN_DELAY else "reference"


def quat_rotation(quat, dtype=np.longdouble):
    """R [..., 3, 3] of the quaternion (x, y, z, w) [..., 4], divided by its norm first."""
    q = np.asarray(quat).astype(dtype)
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    n = np.sqrt(((x * x + y * y) + z * z) + w * w)
    x, y, z, w = x / n, y / n, z / n, w / n
    R = np.empty(q.shape[:-1] + (3, 3), dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = 1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = 2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)
    return R


def measured_pose(meas, params, dtype=np.longdouble, with_status=False):
    """The reference's ``traj_vec`` of a measured state: [..., 18] = CoM (3), Euler angles (3), the feet FL, FR, HL, HR in the
    world (12).

    meas is [..., 18]: base position, Euler angles (roll, pitch, yaw in joints.rotation's convention: the CSV's columns 4 .. 6)
    and q of the twelve joints in csv_entry order; the Euler columns are copied through.  With FLAG_QUAT in params.flags meas is
    [..., 19]: position, the quaternion (x, y, z, w) as Bullet's getBasePositionAndOrientation gives it, q.  The quaternion is
    divided by its norm, R is formed from it directly, and the Euler columns are roll = atan2(R21, R22), pitch =
    asin(clip(-R20, -1, 1)), yaw = atan2(R10, R00); a row where the clip acts (|R20| >= 1) has the status bit GIMBAL.

    Foot e stands at com + R (leg_fk(e, q_e) - (0, 0, ee_shift)): the inverse of towr_transform's lift.  With ee_shift = 0.015
    (joint_params' default) a robot that is exactly on its commanded joint angles and planned pose has zero foot error; with
    ee_shift = 0 the foot is the URDF's FOOT link, which is what the reference's Bullet call returns.

    with_status: returns (pose, status [...] int32 with the GIMBAL bit)."""
    m = np.asarray(meas).astype(dtype)
    quat = bool(int(params.flags) & FLAG_QUAT)
    if m.shape[-1] != (19 if quat else 18):
        raise ValueError("meas is [..., %d]" % (19 if quat else 18))
    pose = np.zeros(m.shape[:-1] + (18,), dtype)
    status = np.zeros(m.shape[:-1], np.int32)
    com = m[..., 0:3]
    pose[..., 0:3] = com
    if quat:
        R = quat_rotation(m[..., 3:7], dtype)
        pose[..., 3] = np.arctan2(R[..., 2, 1], R[..., 2, 2])
        pose[..., 4] = np.arcsin(np.clip(-R[..., 2, 0], dtype(-1), dtype(1)))
        pose[..., 5] = np.arctan2(R[..., 1, 0], R[..., 0, 0])
        status |= np.where(np.abs(R[..., 2, 0]) >= 1, GIMBAL, 0).astype(np.int32)
        q = m[..., 7:19]
    else:
        R = joints.rotation(m[..., 3:6], dtype)
        pose[..., 3:6] = m[..., 3:6]
        q = m[..., 6:18]
    shift = dtype(np.float64(params.ee_shift))
    for e in range(NEE):
        p = joints.leg_fk(e, q[..., 3 * e:3 * e + 3], params, dtype)
        px, py, pz = p[..., 0], p[..., 1], p[..., 2] - shift
        for i in range(3):
            pose[..., 6 + 3 * e + i] = com[..., i] + ((R[..., i, 0] * px + R[..., i, 1] * py) + R[..., i, 2] * pz)
    return (pose, status) if with_status else pose


def errors(ref_rows, pose, dtype=None):
    """Tracking._update's five errors [..., 5]: |ref - meas| of the CoM position and of the feet FL, FR, HL, HR, each
    sqrt((d0 d0 + d1 d1) + d2 d2), one rounded operation after the other.  ref_rows are Cartesian CSV rows [..., >= 19] (columns
    1 .. 3 and 7 .. 18 are read), pose is measured_pose's [..., 18]."""
    ref, pose = np.asarray(ref_rows), np.asarray(pose)
    if dtype is not None:
        ref, pose = ref.astype(dtype), pose.astype(dtype)
    out = []
    for rc, pc in ((1, 0), (7, 6), (10, 9), (13, 12), (16, 15)):
        d0, d1, d2 = (ref[..., rc + i] - pose[..., pc + i] for i in range(3))
        out.append(np.sqrt((d0 * d0 + d1 * d1) + d2 * d2))
    return np.stack(out, -1)


def recorded(call, delay, rule="reference"):
    """Whether the 1-based call number(s) `call` of a window are recorded.  "reference": Tracking.update's branch structure as it
    stands, call >= delay and call != delay + 1 (with delay 500: calls 500, 502, 503, ...; with 0: 2, 3, ...).  "clean":
    call > delay."""
    c = np.asarray(call, np.int64)
    if rule == "reference":
        return (c >= delay) & (c != delay + 1)
    if rule == "clean":
        return c > delay
    raise ValueError("rule is 'reference' or 'clean'")


def accumulate(err, count, total, params):
    """The running totals over the rows' errors err [n, 5] in order: (per-row recorded flags [n], totals [n, 2] after every row,
    count, total).  Row j is call calls + j + 1; a recorded row adds e_com to total_com, then e_FL, e_FR, e_HL, e_HR to
    total_feet, one chain in that order as Tracking._update runs: float64 additions."""
    err = np.asarray(err).astype(np.float64)
    calls, rec = int(count[0]), int(count[1])
    tc, tf = np.float64(total[0]), np.float64(total[1])
    n = len(err)
    flags = recorded(calls + 1 + np.arange(n), int(params.delay), rule_of(params))
    run = np.zeros((n, 2), np.float64)
    for j in range(n):
        if flags[j]:
            tc = tc + err[j, 0]
            tf = tf + err[j, 1]
            tf = tf + err[j, 2]
            tf = tf + err[j, 3]
            tf = tf + err[j, 4]
            rec += 1
        run[j, 0], run[j, 1] = tc, tf
    return flags, run, (calls + n, rec), (float(tc), float(tf))


def plan_positions(L, x, t0, hz, first_row, n_rows, dtype=np.longdouble):
    """Columns 0 .. 18 of the CSV rows first_row .. first_row + n_rows - 1 of a plan, [n_rows, 19] in dtype: the time stamp and the
    positions at min(k / hz, T), as joints.joint_rows takes them."""
    from oracle import splines
    k = np.arange(int(first_row), int(first_row) + int(n_rows))
    tk = k / np.float64(hz)
    t = np.minimum(tk, L.T)
    rows = np.zeros((len(k), 19), dtype)
    rows[:, 0] = dtype(np.float64(t0)) + tk.astype(dtype)
    rows[:, 1:4], rows[:, 4:7] = splines.eval_spline(L, 0, x, t, 0, dtype), splines.eval_spline(L, 1, x, t, 0, dtype)
    for e in range(NEE):
        rows[:, 7 + 3 * e:10 + 3 * e] = splines.eval_spline(L, 2 + e, x, t, 0, dtype)
    return rows


def track_rows(L, x, t0, hz, first_row, n_rows, meas, params, count=(0, 0), total=(0.0, 0.0), goal_x=None, dtype=np.longdouble):
    """The track rows first_row .. first_row + n_rows - 1 of a plan against the measured states meas [n_rows, 18 | 19]:
    (rows [n_rows, 26] in dtype, status [n_rows] int32, count, total).  Column 0 is the time stamp of CSV row k, columns 1 .. 18
    measured_pose, 19 .. 23 the errors against the plan's own row k (positions at min(k / hz, T)), 24 total_com and 25 total_feet
    after this row.  count = (calls, recorded) and total = (total_com, total_feet) come in and go out; unrecorded rows carry
    their pose and errors and repeat the standing totals.  Status bits: RECORDED; REACHED, measured com x >= goal_x (None:
    never); GIMBAL."""
    n = int(n_rows)
    if n <= 0:
        return np.zeros((0, TRACK_COLS), dtype), np.zeros(0, np.int32), (int(count[0]), int(count[1])), (float(total[0]), float(total[1]))
    ref = plan_positions(L, x, t0, hz, first_row, n, dtype)
    m = np.asarray(meas)
    pose, status = measured_pose(m[:n], params, dtype, with_status=True)
    err = errors(ref, pose)
    flags, run, count, total = accumulate(err, count, total, params)
    out = np.zeros((n, TRACK_COLS), dtype)
    out[:, 0], out[:, 1:19], out[:, 19:24], out[:, 24:26] = ref[:, 0], pose, err, run.astype(dtype)
    status = status | np.where(flags, RECORDED, 0).astype(np.int32)
    if goal_x is not None:
        status = status | np.where(np.asarray(m[:n, 0], np.float64) >= np.float64(goal_x), REACHED, 0).astype(np.int32)
    return out, status.astype(np.int32), count, total


def track_ring(L, x, t0, hz, first_row, n_rows, meas_ring, cursor, params, out_ring, status_ring, count=(0, 0), total=(0.0, 0.0),
               goal_x=None, dtype=np.longdouble):
    """track_rows with k_stitch's addressing (stitcher.ring_append): row first_row + j reads meas_ring[(cursor + j) % capacity] and
    goes to the same row of out_ring [capacity, 26] and status_ring [capacity], in place; n_rows is clamped to 0 .. capacity and
    the cursor is only read.  Returns (count, total)."""
    cap = len(out_ring)
    n = min(max(int(n_rows), 0), cap)
    at = ring_index(cursor, n, cap)
    rows, status, count, total = track_rows(L, x, t0, hz, first_row, n, np.asarray(meas_ring)[at], params, count, total, goal_x, dtype)
    out_ring[at] = rows
    status_ring[at] = status
    return count, total
