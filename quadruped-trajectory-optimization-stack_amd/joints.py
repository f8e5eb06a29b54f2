"""Joint commands of a plan: the rule of k_joint_rows (qtos_joint_rows*, include/qtos_planner.h) stated in numpy.

What the reference's consumer does once per 1 kHz tick (scripts/run.py:184-200, QTOS/robot/robot.py control_multi):

  * ``towr_transform`` (QTOS/utils.py:412-436): the planned feet in the base frame of the planned pose, lifted by ee_shift
  * inverse kinematics per leg (the reference asks PyBullet; the SOLO12 leg has a closed form, below)
  * ``MotorModel.convert_to_torque*`` (QTOS/robot/robot_motor.py): PD plus feed-forward, clipped

The number type is a parameter, as in oracle/splines.py: dtype = np.longdouble is what the kernel is held to, np.float64 the
same formulas in the kernel's own precision.

The leg (data/urdf/solo12.urdf): HAA about x at ``hip``, then HFE and KFE about y, the three y offsets behind the HAA add up
to the lateral offset d, the links are l_u and l_l long and point down at q = 0.  With the hip frame the frame behind the
HAA rotation, the foot stands at u = (x, d, -h) in it,

    x = -l_u sin q2 - l_l sin(q2 + q3)        h = l_u cos q2 + l_l cos(q2 + q3)

and at p = hip + Rx(q1) u in the base frame: r = p - hip has r_y = d cos q1 + h sin q1, r_z = d sin q1 - h cos q1, hence
h^2 = r_y^2 + r_z^2 - d^2, r_y h + r_z d = (h^2 + d^2) sin q1 and r_y d - r_z h = (h^2 + d^2) cos q1; x^2 + h^2 =
l_u^2 + l_l^2 + 2 l_u l_l cos q3, and the direction of (h, -x) is q2 plus the angle of (l_u + l_l cos q3, l_l sin q3).
With rho^2 = x^2 + h^2: 1 - cos q3 = ((l_u + l_l)^2 - rho^2) / (2 l_u l_l) and 1 + cos q3 = (rho^2 - (l_u - l_l)^2) / (2 l_u l_l), whose
square roots are in the ratio tan(q3 / 2): what leg_ik forms the knee from on the fold side.
"""
import numpy as np

NEE = 4
LEGS = ("FL", "FR", "HL", "HR")            # the order of SOLO12.csv_entry
JOINTS = ("HAA", "HFE", "KFE")
JOINT_COLS = 37
REACH, FOLD, INSIDE = 1, 2, 4              # status bits of one leg (leg_ik)
NONFINITE = 8                              # of one leg: the target, or one of the leg's numbers, is not finite (bit 12 + e of a row)
STATUS_NONFINITE = 1 << 12                 # QTOS_JOINT_NONFINITE: leg 0's bit in the status word of a row
FLAG_NO_FF = 1                             # QtosJointRows.flags bit 0: the feed-forward torque is left out (convert_to_torque)


class Solo12:
    """The leg data of data/urdf/solo12.urdf, typed in once, digit for digit: the file writes 0.0875 and 0.03745 one unit in the
    last place up, and the doubles here are the doubles a URDF parser reads."""
    _Y, _D = 0.08750000000000001, 0.014 + 0.037450000000000004 + 0.008      # HAA y; HFE y + KFE y + ANKLE y
    hip = np.array([[0.1946, _Y, 0.0], [0.1946, -_Y, 0.0], [-0.1946, _Y, 0.0], [-0.1946, -_Y, 0.0]])
    lateral = np.array([_D, -_D, _D, -_D])
    l_upper = 0.16
    l_lower = 0.16
    knee_sign = np.array([-1.0, -1.0, 1.0, 1.0])     # the branch of q_init in data/config/solo12.yml: front knees back, hind knees forward


SOLO12 = Solo12()


class JointParams:
    """What joint_rows reads: the leg data, ee_shift and the motor law.  capi.QtosJointRows has the same field names and is
    taken as well."""

    def __init__(self, robot=SOLO12, ee_shift=0.015, kp=20.0, kd=0.08, hip_scale=1.0, knee_scale=1.0, ankle_scale=1.0, tau_max=8.0,
                 flags=0):
        self.hip, self.lateral = np.array(robot.hip, np.float64), np.array(robot.lateral, np.float64)
        self.l_upper, self.l_lower = float(robot.l_upper), float(robot.l_lower)
        self.knee_sign = np.array(robot.knee_sign, np.float64)
        self.ee_shift = float(ee_shift)
        self.kp, self.kd = motor_gains(kp, kd, hip_scale, knee_scale, ankle_scale)
        self.tau_max = float(tau_max)
        self.flags = int(flags)


def _field(params, name, shape=None):
    a = np.array(getattr(params, name), np.float64)
    return a if shape is None else a.reshape(shape)


def rotation(euler, dtype=np.longdouble):
    """R = Rz(yaw) Ry(pitch) Rx(roll) of euler = (roll, pitch, yaw) [..., 3]: scipy's from_euler('xyz'), [..., 3, 3]."""
    e = np.asarray(euler).astype(dtype)
    sa, ca, sb, cb, sc, cc = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1]), np.sin(e[..., 2]), np.cos(e[..., 2])
    R = np.empty(e.shape[:-1] + (3, 3), dtype)
    R[..., 0, 0], R[..., 0, 1], R[..., 0, 2] = cc * cb, cc * sb * sa - sc * ca, cc * sb * ca + sc * sa
    R[..., 1, 0], R[..., 1, 1], R[..., 1, 2] = sc * cb, sc * sb * sa + cc * ca, sc * sb * ca - cc * sa
    R[..., 2, 0], R[..., 2, 1], R[..., 2, 2] = -sb, cb * sa, cb * ca
    return R


def rotation_rate(euler, euler_rate, dtype=np.longdouble):
    """The time derivative of rotation(euler) with the Euler rates euler_rate: the product rule on Rz Ry Rx, entry by entry."""
    e, w = np.asarray(euler).astype(dtype), np.asarray(euler_rate).astype(dtype)
    sa, ca, sb, cb, sc, cc = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1]), np.sin(e[..., 2]), np.cos(e[..., 2])
    # d/dt of the sines and cosines
    dsa, dca, dsb, dcb, dsc, dcc = ca * w[..., 0], -sa * w[..., 0], cb * w[..., 1], -sb * w[..., 1], cc * w[..., 2], -sc * w[..., 2]
    D = np.empty(e.shape[:-1] + (3, 3), dtype)
    D[..., 0, 0] = dcc * cb + cc * dcb
    D[..., 0, 1] = dcc * sb * sa + cc * dsb * sa + cc * sb * dsa - dsc * ca - sc * dca
    D[..., 0, 2] = dcc * sb * ca + cc * dsb * ca + cc * sb * dca + dsc * sa + sc * dsa
    D[..., 1, 0] = dsc * cb + sc * dcb
    D[..., 1, 1] = dsc * sb * sa + sc * dsb * sa + sc * sb * dsa + dcc * ca + cc * dca
    D[..., 1, 2] = dsc * sb * ca + sc * dsb * ca + sc * sb * dca - dcc * sa - cc * dsa
    D[..., 2, 0] = -dsb
    D[..., 2, 1] = dcb * sa + cb * dsa
    D[..., 2, 2] = dcb * ca + cb * dca
    return D


def _rt(R, v):
    """R^T v over leading axes."""
    return np.einsum("...ji,...j->...i", R, v)


def base_frame(com, euler, foot, ee_shift, com_vel=None, euler_rate=None, foot_vel=None, dtype=np.longdouble):
    """towr_transform: the foot in the base frame of the planned pose, p_b = R(euler)^T (foot - com) + (0, 0, ee_shift), and its
    time derivative v_b = dR^T/dt (foot - com) + R^T (foot_vel - com_vel) from the plan's own velocities (None without
    them).  All [..., 3]; returns (p_b, v_b)."""
    com, foot = np.asarray(com).astype(dtype), np.asarray(foot).astype(dtype)
    R = rotation(euler, dtype)
    d = foot - com
    p_b = _rt(R, d)
    p_b[..., 2] = p_b[..., 2] + dtype(ee_shift)
    if com_vel is None:
        return p_b, None
    D = rotation_rate(euler, euler_rate, dtype)
    v_b = _rt(D, d) + _rt(R, np.asarray(foot_vel).astype(dtype) - np.asarray(com_vel).astype(dtype))
    return p_b, v_b


def ik_margins(leg, p_b, robot=SOLO12, dtype=np.longdouble):
    """(c3, h2) of leg_ik: the knee's cosine before it is clipped and the squared depth of the foot under the hip axis.  The
    status bits are c3 > 1, c3 < -1 and h2 < 0."""
    hip, d = _field(robot, "hip", (NEE, 3))[leg].astype(dtype), dtype(_field(robot, "lateral")[leg])
    lu, ll = dtype(robot.l_upper), dtype(robot.l_lower)
    r = np.asarray(p_b).astype(dtype) - hip
    h2 = r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2] - d * d
    c3 = (r[..., 0] * r[..., 0] + np.maximum(h2, dtype(0)) - lu * lu - ll * ll) / (2 * lu * ll)
    return c3, h2


def leg_ik(leg, p_b, robot=SOLO12, dtype=np.longdouble):
    """Closed-form inverse kinematics of leg `leg` (0 FL, 1 FR, 2 HL, 3 HR) for the foot at p_b [..., 3] in the base frame:
    (q [..., 3] = HAA, HFE, KFE, status [...] int32).  Status bits: REACH (c3 > 1: the target is beyond the leg's length; the
    leg is straight and points at it, the nearest reachable point in the leg's plane), FOLD (c3 < -1) and INSIDE (h^2 < 0: the
    target is nearer to the hip axis than the lateral offset; h is taken as 0).  The two clips keep a NaN (np.maximum, np.clip),
    and a target with a non-finite component has q = (NaN, NaN, NaN) and the bit NONFINITE: no finite angle comes out of a
    target that is not a point (the formulas alone would give a NaN in r_x the q1 of the other two components, and an
    infinite r_z the angles of a leg that points at it).  The three comparisons are what they are on such a target."""
    hip, d = _field(robot, "hip", (NEE, 3))[leg].astype(dtype), dtype(_field(robot, "lateral")[leg])
    lu, ll, knee = dtype(robot.l_upper), dtype(robot.l_lower), dtype(_field(robot, "knee_sign")[leg])
    r = np.asarray(p_b).astype(dtype) - hip
    rx, ry, rz = r[..., 0], r[..., 1], r[..., 2]
    c3, h2 = ik_margins(leg, p_b, robot, dtype)
    h = np.sqrt(np.maximum(h2, dtype(0)))
    q3 = knee * np.arccos(np.clip(c3, dtype(-1), dtype(1)))
    # The fold side, c3 < -1/2.  There c3 + 1 = (rho^2 - (l_u - l_l)^2) / (2 l_u l_l), rho^2 = r_x^2 + h^2, is a small number next
    # to 1 and h^2 a small difference of squares, so c3 and the h above resolve a foot next to the folded length only to
    # nanometres.  h^2 is formed as (r_y - d)(r_y + d) + r_z^2 and the knee from the half angle, tan(q3 / 2) =
    # sqrt((1 - c3) / (1 + c3)), with both numerators formed from rho^2 directly.  The status bits stay the comparisons of
    # c3 and h^2 as ik_margins forms them: a leg with INSIDE keeps h = 0, one with FOLD q3 = +-pi.
    with np.errstate(invalid="ignore"):
        fold = c3 < -0.5
        hf = np.where(h2 < 0, dtype(0), np.sqrt(np.maximum((ry - d) * (ry + d) + rz * rz, dtype(0))))
        rho2 = rx * rx + hf * hf
        a = np.maximum(((lu + ll) * (lu + ll) - rho2) / (2 * lu * ll), dtype(0))
        b = np.where(c3 < -1, dtype(0), np.maximum((rho2 - (lu - ll) * (lu - ll)) / (2 * lu * ll), dtype(0)))
        h = np.where(fold, hf, h)
        q3 = np.where(fold, knee * (2 * np.arctan2(np.sqrt(a), np.sqrt(b))), q3)
    q1 = np.arctan2(ry * h + rz * d, ry * d - rz * h)
    q2 = np.arctan2(-rx, h) - np.arctan2(ll * np.sin(q3), lu + ll * np.cos(q3))
    bad = ~np.isfinite(r).all(-1)
    status = (REACH * (c3 > 1) + FOLD * (c3 < -1) + INSIDE * (h2 < 0) + NONFINITE * bad).astype(np.int32)
    return np.where(bad[..., None], dtype(np.nan), np.stack([q1, q2, q3], -1)), status


def _hip_frame(leg, q, robot, dtype):
    """What the chain's Jacobian is made of at q: (s1, c1, x, h, l_l sin(q2 + q3), l_l cos(q2 + q3), d, l_u l_l sin q3)."""
    d = dtype(_field(robot, "lateral")[leg])
    lu, ll = dtype(robot.l_upper), dtype(robot.l_lower)
    q = np.asarray(q).astype(dtype)
    s1, c1, s2, c2 = np.sin(q[..., 0]), np.cos(q[..., 0]), np.sin(q[..., 1]), np.cos(q[..., 1])
    s23, c23 = np.sin(q[..., 1] + q[..., 2]), np.cos(q[..., 1] + q[..., 2])
    x = -lu * s2 - ll * s23
    h = lu * c2 + ll * c23
    return s1, c1, x, h, ll * s23, ll * c23, d, lu * ll * np.sin(q[..., 2])


def leg_fk(leg, q, robot=SOLO12, dtype=np.longdouble):
    """The foot of leg `leg` at q [..., 3], in the base frame: hip + Rx(q1) (x, d, -h)."""
    hip = _field(robot, "hip", (NEE, 3))[leg].astype(dtype)
    s1, c1, x, h, _, _, d, _ = _hip_frame(leg, q, robot, dtype)
    return np.stack([hip[0] + x, hip[1] + c1 * d + s1 * h, hip[2] + s1 * d - c1 * h], -1)


def leg_jacobian(leg, q, robot=SOLO12, dtype=np.longdouble):
    """d foot / d q of leg_fk, [..., 3, 3] in the base frame: Rx(q1) times the hip-frame columns (0, h, d), (-h, 0, -x) and
    (-l_l cos(q2 + q3), 0, l_l sin(q2 + q3))."""
    s1, c1, x, h, ls, lc, d, _ = _hip_frame(leg, q, robot, dtype)
    J = np.zeros(np.shape(x) + (3, 3), dtype)
    J[..., 1, 0], J[..., 2, 0] = c1 * h - s1 * d, s1 * h + c1 * d
    J[..., 0, 1], J[..., 1, 1], J[..., 2, 1] = -h, s1 * x, -c1 * x
    J[..., 0, 2], J[..., 1, 2], J[..., 2, 2] = -lc, -s1 * ls, c1 * ls
    return J


def joint_rates(leg, q, v_b, status=None, robot=SOLO12, dtype=np.longdouble):
    """qdot = J^-1 v_b by a closed solve in the hip frame: with w = Rx(q1)^T v_b, w_y = h qdot1, and the 2 x 2 system of
    (w_x, w_z - d qdot1) in (qdot2, qdot3) has the determinant -l_u l_l sin q3.  A leg with a status bit gets qdot = 0 (J is
    singular at a straight or folded knee and at h = 0); a leg with leg_ik's NONFINITE bit gets qdot = NaN."""
    s1, c1, x, h, ls, lc, d, det = _hip_frame(leg, q, robot, dtype)
    v = np.asarray(v_b).astype(dtype)
    wx, wy, wz = v[..., 0], c1 * v[..., 1] + s1 * v[..., 2], c1 * v[..., 2] - s1 * v[..., 1]
    st = np.zeros(np.shape(x), np.int32) if status is None else np.asarray(status)
    ok = (st & (REACH | FOLD | INSIDE)) == 0
    hs, dets = np.where(ok, h, dtype(1)), np.where(ok, -det, dtype(1))
    qd1 = wy / hs
    rz = wz - d * qd1
    qd2 = (wx * ls + lc * rz) / dets
    qd3 = (x * wx - h * rz) / dets
    qd = np.where(ok[..., None], np.stack([qd1, qd2, qd3], -1), dtype(0))
    return np.where(((st & NONFINITE) != 0)[..., None], dtype(np.nan), qd)


def feed_forward(leg, q, euler, force, robot=SOLO12, dtype=np.longdouble):
    """tau_ff = -J^T R(euler)^T f, f the plan's force on the foot in the world frame: the joint torques that push the foot
    against the ground with f."""
    s1, c1, x, h, ls, lc, d, _ = _hip_frame(leg, q, robot, dtype)
    fb = _rt(rotation(euler, dtype), np.asarray(force).astype(dtype))
    gx, gy, gz = fb[..., 0], c1 * fb[..., 1] + s1 * fb[..., 2], c1 * fb[..., 2] - s1 * fb[..., 1]
    return np.stack([-(h * gy + d * gz), h * gx + x * gz, lc * gx - ls * gz], -1)


def motor_gains(kp, kd, hip=1.0, knee=1.0, ankle=1.0):
    """MotorModel.UPDATE_GAIT for both gains: (kp [12], kd [12]), each gain scaled per joint of every leg."""
    out = []
    for gain in (kp, kd):
        g = np.ones(3 * NEE) * gain
        g[0::3] *= hip
        g[1::3] *= knee
        g[2::3] *= ankle
        out.append(g)
    return out[0], out[1]


def motor_torque(q, qd, tau_ff, kp, kd, tau_max, q_mes=None, qd_mes=None):
    """MotorModel.convert_to_torque_ff: clip(kp (q - q_mes) + kd (qd - qd_mes) + tau_ff, -tau_max, tau_max) in the arrays' own
    type, one rounded operation after the other.  Without measured values the PD terms are left out; tau_max <= 0: no clip;
    tau_ff None: without feed-forward (convert_to_torque)."""
    q, qd = np.asarray(q), np.asarray(qd)
    if q_mes is None:
        tau = np.zeros_like(q) if tau_ff is None else np.array(tau_ff)
    else:
        tau = np.asarray(kp) * (q - np.asarray(q_mes)) + np.asarray(kd) * (qd - np.asarray(qd_mes))
        if tau_ff is not None:
            tau = tau + np.asarray(tau_ff)
    return np.clip(tau, -tau_max, tau_max) if tau_max > 0 else tau


def joint_state(rows, foot_vel, params, dtype=np.longdouble):
    """Cartesian rows [n, 37] (in dtype) and the feet's velocities [n, 4, 3] -> (q [n, 12], qd [n, 12], tau_ff [n, 12],
    status [n] int32: bit e reach, bit 4 + e fold, bit 8 + e inside of foot e, bit 12 + e nonfinite: one of the leg's nine
    numbers q, qdot, tau_ff -- tau_ff as the motor law takes it, 0 with FLAG_NO_FF -- is not finite)."""
    n = rows.shape[0]
    no_ff = bool(int(getattr(params, "flags", 0)) & FLAG_NO_FF)
    q, qd, tff = np.zeros((n, 12), dtype), np.zeros((n, 12), dtype), np.zeros((n, 12), dtype)
    status = np.zeros(n, np.int32)
    for e in range(NEE):
        p_b, v_b = base_frame(rows[:, 1:4], rows[:, 4:7], rows[:, 7 + 3 * e:10 + 3 * e], params.ee_shift, rows[:, 19:22],
                              rows[:, 22:25], foot_vel[:, e], dtype)
        qe, st = leg_ik(e, p_b, params, dtype)
        q[:, 3 * e:3 * e + 3] = qe
        qd[:, 3 * e:3 * e + 3] = joint_rates(e, qe, v_b, st, params, dtype)
        tff[:, 3 * e:3 * e + 3] = feed_forward(e, qe, rows[:, 4:7], rows[:, 25 + 3 * e:28 + 3 * e], params, dtype)
        status |= ((st & REACH) << e) | (((st & FOLD) >> 1) << (4 + e)) | (((st & INSIDE) >> 2) << (8 + e))
        nine = [q[:, 3 * e:3 * e + 3], qd[:, 3 * e:3 * e + 3]] + ([] if no_ff else [tff[:, 3 * e:3 * e + 3]])
        bad = ~np.isfinite(np.concatenate(nine, 1)).all(1)
        status |= np.where(bad, STATUS_NONFINITE << e, 0).astype(np.int32)
    return q, qd, tff, status


def joint_rows(L, x, t0, hz, first_row, n_rows, params, q_mes=None, qd_mes=None, dtype=np.longdouble):
    """The joint rows first_row .. first_row + n_rows - 1 of a plan: ([n_rows, 37] in dtype, status [n_rows] int32).  Column 0 is
    the time stamp of CSV row k, t0 + k / hz, columns 1 .. 12 q, 13 .. 24 qdot, 25 .. 36 tau (leg order FL, FR, HL, HR, joint
    order HAA, HFE, KFE), at the plan time k_sample uses for row k: min(k / hz, T).  L is the plan's oracle.splines.layout, x
    its nodes; the feet's velocities are the foot splines' first derivatives."""
    from oracle import splines
    k = np.arange(int(first_row), int(first_row) + int(n_rows))
    tk = k / np.float64(hz)
    t = np.minimum(tk, L.T)
    rows = np.zeros((len(k), 37), dtype)
    rows[:, 0] = dtype(np.float64(t0)) + tk.astype(dtype)
    rows[:, 1:4], rows[:, 4:7] = splines.eval_spline(L, 0, x, t, 0, dtype), splines.eval_spline(L, 1, x, t, 0, dtype)
    rows[:, 19:22], rows[:, 22:25] = splines.eval_spline(L, 0, x, t, 1, dtype), splines.eval_spline(L, 1, x, t, 1, dtype)
    fv = np.zeros((len(k), NEE, 3), dtype)
    for e in range(NEE):
        rows[:, 7 + 3 * e:10 + 3 * e] = splines.eval_spline(L, 2 + e, x, t, 0, dtype)
        rows[:, 25 + 3 * e:28 + 3 * e] = splines.eval_spline(L, 6 + e, x, t, 0, dtype)
        fv[:, e] = splines.eval_spline(L, 2 + e, x, t, 1, dtype)
    q, qd, tff, status = joint_state(rows, fv, params, dtype)
    out = np.zeros((len(k), JOINT_COLS), dtype)
    out[:, 0], out[:, 1:13], out[:, 13:25] = rows[:, 0], q, qd
    mes = None if q_mes is None else np.asarray(q_mes).astype(dtype)
    dmes = None if qd_mes is None else np.asarray(qd_mes).astype(dtype)
    ff = None if int(getattr(params, "flags", 0)) & FLAG_NO_FF else tff
    out[:, 25:37] = motor_torque(q, qd, ff, _field(params, "kp").astype(dtype), _field(params, "kd").astype(dtype),
                                 dtype(params.tau_max), mes, dmes)
    return out, status
