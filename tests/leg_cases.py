"""Shared by test_leg_cpu.py and test_gpu_leg.py: the probe table the three hand-written copies of the SOLO12 leg chain (joint_leg in
k_joint_rows, track_leg in k_track and k_start_feedback, fit_foot_out in k_force_fit and k_force_qp; csrc/window_kernels.hpp) are
held to the statements (qtos_amd/joints.py, qtos_amd/tracking.py) and to the URDF's chain (tests/joint_chain.py) on, the hand-written
pose plans that put a planner's windows on those probes, the gates and the accuracy record.  No tests in here.

Pose plans.  The kernels read a plan's nodes as data, so pose_nodes() writes one by hand: every position node of the base's two
splines is p + v t_node with the velocity node v, every node of foot e is feet[e] with velocity 0, every force node forces[e].
On the smallest transcription (CFG: 1 s, 0.5 s steps, 464 variables) every position node has a variable, row 0 of the sampled
plan is the pose to the bit, and a static pose (all velocities 0) is every row whose plan time is 0 or T: between the nodes the
Hermite weights of the numpy sampler leave a constant foot a unit in the last place off.  So the windows are sampled at HZ = 1:
row 0 at t = 0 and every later row at min(k / HZ, T) = T, and a static probe's 65 sampled rows are its row 0 to the bit.  (The
kernels' evaluator of the feet's velocities is not part of that: it leaves 1e-30 m/s on a constant foot at t = T, which reaches
the rates of the rows behind row 0, so those are held to one another, not to row 0.)  A probe is row 0 of its window.

Probes.  A probe gives every leg the same target r relative to its hip, mirrored in y for the right legs (d = lateral[e], so
r_y = d means "under the hip axis by the lateral offset"), at identity attitude with the CoM at the origin unless it says
otherwise: there R is exactly the identity, p_b is the foot itself, and the float64 statement and the kernel see the same bits
of c3 and h^2 (the kernel's lines are compiled without contraction).  The world foot is hip + r - (0, 0, ee_shift) formed in
longdouble and rounded once; the r a leg then sees, ((foot_z + ee_shift) - hip_z and so on), is off the nominal r by a rounding
or two, which is why the thresholds are found by stepping the foot's coordinate in units in the last place and asking the
float64 statement on which side each step lies (stepped()).  Classes:

  stretch_down      r = (0, d, -(l_u + l_l)) and the foot's z stepped -8 .. 8 units in the last place: c3 on both sides of 1
  stretch_exact     the same with y stepped as well: the first (y, z) step in -8 .. 8 at which the float64 c3 == 1 on every leg;
                    absent, and EXACT["c3 == 1"] False, where no step attains it
  stretch_x+ / x-   r = (+-(l_u + l_l), d, 0)
  beyond            1.5 x the stretch: REACH, the leg is straight and points at the target
  near_straight_k   c3 = 1 - 10^-k, k = 4, 8, 12, straight down
  near_fold_k       r = (0, d, -10^-k), k = 3, 8, and r_z = 0: with equal links c3 >= -1 always
  inside            r = (0.1, d / 2, 0): INSIDE, and inside_x0 with r_x = 0, where both arguments of q2's first atan2 are zero;
                    inside_h2- / h2+ the two sides of h^2 = 0 at r = (0.1, d, 0), y stepped;
                    inside_h2=0 where a step gives h^2 == 0 exactly (else EXACT["h2 == 0"] is False)
  quadrant_*        above the hip axis (r_z > 0), level with it outwards and inwards, behind and under it: q1 in all four quadrants
                    per leg.  The other two atan2 calls have a first argument of either sign but a second one >= 0 (h is a
                    square root, l_u + l_l cos q3 >= 0 with equal links): both of their reachable quadrants occur (r_x of both
                    signs, both knee branches)
  attitude_*        the nominal stance r = (0, d, -0.24) in the base frame under seven attitudes, among them +-pi about every
                    axis, +-pi / 2 of pitch and two generic ones with angles beyond pi; CoM off the origin
  moving_*          four of the above with a CoM velocity and Euler rates, two sets
  nonfinite_*       NaN and +inf in each coordinate of one foot (leg 1), in the CoM, in one Euler angle, in one force (leg 2)
  fold_*            (FOLD_PROBES, their own launch: JointParams with l_upper 0.17, l_lower 0.15) a target 0.01 from the hip's
                    pitch axis: the only way to the FOLD bit; the two sides of c3 = -1 at 0.02, z stepped 16 units at a time; an unflagged one
Angle probes (the forward chain and the torque chain): every triple of {0, +-pi/2, +-pi, 7.0, -9.5} and the inverse
kinematics' own angles of the finite probes.  Quaternion probes: unit, norm 3, pitch exactly +-pi / 2, zero, NaN, inf.

Gates.  u = 2^-53; as tests/test_gpu_joints.py and tests/test_gpu_track.py state, 4 ulp are ASSUMED for each of the device's sqrt, sin,
cos, atan2, acos and asin, and every gate is capped at 1e-12.  No gate is taken from a kernel's output; where a gate has a
floor it is the float64 statement's distance from its longdouble form at the same probe, with the project's factor 8.

  angles, identity   against the float64 statement on the same input bits.  c3, h and both arguments of every atan2 are then
                     the same doubles on both sides, so only the library calls differ.  One ulp of a result below pi is 4 u, so
                     the device's 4 ulp and the host's 1 are 20 u per call: q3 = acos: 20 u; q1 = one atan2: 20 u; q2 = two
                     atan2 (40 u), the second of which reads the sine and cosine (4 ulp of a value below 1: 8 u each) of a q3 that
                     is 20 u off, half of which reaches q2: 40 + 16 + 10 = 66 u.  Taken as 256 u rad, ANGLE_SAME_BITS
  angles, other      against the longdouble statement: (128 + 140 / |sin q3|) u, tests/test_gpu_joints.py's derivation
  FK round trip      joint_chain.chain at the kernel's angles against p_b (REACH: against the nearest reachable point, the foot
                     of the straight leg): max(8 x floor, 64 u m)
  rates              |J_geo(q_gpu) qdot - v_b| <= max(8 x floor, 64 u (1 + 0.5 |qdot|_inf)): the residual of a solve with the
                     levers of 0.5 m at most grows with the rate near the knee's singularity, so this gate alone is not capped
                     (at |qdot| = 2.9e5 rad/s, c3 = 1 - 1e-8, the float64 statement's own residual is 1.0e-12)
  torques            |tau + J_geo^T R^T f| <= max(8 x floor, 64 u |f|_1 0.5 m)
  track              FEET_BOUND = 128 u m and EULER_BOUND = 256 u rad of tests/test_gpu_track.py
"""
import json
import os

import numpy as np

from conftest import ROOT  # noqa: F401  (path set-up)

import joint_chain as jc
import plan_check_cases as pcc

LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
CAP = 1e-12
MARGIN = 1e-12                       # off identity attitude the status is compared where c3 -+ 1 and h^2 are further than this from 0
ANGLE_SAME_BITS = 256 * U
FK_BOUND, RATE_BOUND, TORQUE_BOUND = 64 * U, 64 * U, 64 * U * 0.5
FEET_BOUND, EULER_BOUND = 128 * U, 256 * U
ROUND_TRIP_BOUND = 128 * U           # k_joint_rows' angles through k_track's chain: the foot error columns
EE_SHIFT = 0.015
HZ, TILE_ROWS = 1.0, 65              # rows at t = 0, T, T, ...; 65 rows: one more than the one-wave kernel takes
STEPS = 8                            # units in the last place searched on either side of a threshold
FOLD_STEP = 16                       # the fold threshold's probes are this many units apart
FORCES = np.array([[1.0, 2.0, 9.0], [-1.0, 0.5, 8.0], [0.3, 0.2, 7.0], [0.0, -2.0, 6.0]])
VELOCITIES = (((0.3, -0.2, 0.1), (0.3, -0.2, 0.1)), ((1.5, -2.0, 2.5), (1.5, -2.0, 2.5)))      # (com_vel, euler_rate)
ATTITUDES = ((0.0, 0.0, np.pi), (0.0, 0.0, -np.pi), (0.0, np.pi / 2, 0.0), (0.0, -np.pi / 2, 0.0), (np.pi, 0.0, 0.0),
             (2.5, -1.2, 4.0), (7.0, -8.0, 9.0))
ATTITUDE_COM = (0.3, -0.2, 0.31)
ANGLE_VALUES = (0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, 7.0, -9.5)
TRACK_POSE = ((0.3, -0.2, 0.31), (0.4, -1.1, 2.5))                                               # measured CoM and Euler angles of the angle rows
EXACT = {}                           # "c3 == 1", "h2 == 0": whether a float64 within the searched steps attains it (filled by probes())
_cache = {}


def cfg():
    from qtos_amd.config import PlannerConfig
    return PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5)


def layout():
    if "L" not in _cache:
        from oracle import splines as sp
        _cache["L"] = sp.layout(cfg())
    return _cache["L"]


def pose_nodes(L, com, euler, com_vel, euler_rate, feet, forces):
    """The nodes of a plan that is the pose at t = 0 and moves its base at constant velocities: [L.n_vars] float64."""
    x = np.zeros(L.n_vars)
    base = ((np.asarray(com, F64), np.asarray(com_vel, F64)), (np.asarray(euler, F64), np.asarray(euler_rate, F64)))
    feet, forces = np.asarray(feet, F64).reshape(4, 3), np.asarray(forces, F64).reshape(4, 3)
    with np.errstate(invalid="ignore"):
        for k, S in enumerate(L.splines):
            idx = np.asarray(S.idx).reshape(S.n_polys + 1, 2, 3)
            tn = pcc.node_times(S)
            for n in range(S.n_polys + 1):
                for d in range(3):
                    if k < 2:
                        p, v = base[k][0][d] + base[k][1][d] * tn[n], base[k][1][d]
                    elif k < 6:
                        p, v = feet[k - 2][d], 0.0
                    else:
                        p, v = forces[k - 6][d], 0.0
                    if idx[n, 0, d] >= 0:
                        x[idx[n, 0, d]] = p
                    else:
                        assert k >= 6, "a position node without a variable"
                    if idx[n, 1, d] >= 0:
                        x[idx[n, 1, d]] = v
    return x


class FoldRobot:
    """SOLO12 with unequal links: the folded length |l_u - l_l| = 0.02 m is a sphere a target can lie inside."""
    def __init__(self):
        from qtos_amd import joints
        s = joints.SOLO12
        self.hip, self.lateral, self.knee_sign = s.hip, s.lateral, s.knee_sign
        self.l_upper, self.l_lower = 0.17, 0.15


def robot(name):
    from qtos_amd import joints
    return joints.SOLO12 if name == "solo12" else FoldRobot()


def statement_params(name="solo12", **kw):
    from qtos_amd import joints
    return joints.JointParams(robot=robot(name), ee_shift=EE_SHIFT, **kw)


class Probe:
    """One pose: name, class, robot, the pose and its velocities, the four feet in the world and their forces (float64: what
    the nodes carry), whether it stands at identity attitude, whether all of it is finite, and which legs a non-finite number
    reaches (bad_q: the target; bad_tau: the force only)."""

    def __init__(self, name, cls, feet, com=(0.0, 0.0, 0.0), euler=(0.0, 0.0, 0.0), com_vel=(0.0, 0.0, 0.0), euler_rate=(0.0, 0.0, 0.0),
                 forces=FORCES, robot_name="solo12", bad_q=(), bad_tau=()):
        self.name, self.cls, self.robot_name = name, cls, robot_name
        self.com, self.euler = np.array(com, F64), np.array(euler, F64)
        self.com_vel, self.euler_rate = np.array(com_vel, F64), np.array(euler_rate, F64)
        self.feet, self.forces = np.array(feet, F64).reshape(4, 3), np.array(forces, F64).reshape(4, 3)
        self.identity = not self.com.any() and not self.euler.any() and not self.com_vel.any() and not self.euler_rate.any()
        self.static = not self.com_vel.any() and not self.euler_rate.any()
        self.bad_q, self.bad_tau = tuple(bad_q), tuple(bad_tau)
        self.finite = not self.bad_q and not self.bad_tau

    def nodes(self, L=None):
        return pose_nodes(layout() if L is None else L, self.com, self.euler, self.com_vel, self.euler_rate, self.feet, self.forces)

    def moved(self, name, cls, com_vel, euler_rate):
        return Probe(name, cls, self.feet, self.com, self.euler, com_vel, euler_rate, self.forces, self.robot_name)


def mirrored(r, e, rob):
    """The target r = (r_x, a, r_z, b) of leg e: r_y = a d + b sign(d), d the leg's lateral offset."""
    d = LD(rob.lateral[e])
    return np.array([LD(r[0]), LD(r[1]) * d + LD(r[3] if len(r) > 3 else 0.0) * np.sign(d), LD(r[2])], LD)


def world_feet(r, rob, com=(0.0, 0.0, 0.0), euler=(0.0, 0.0, 0.0)):
    """The four feet in the world whose targets in the base frame are hip + r: com + R (hip + r - (0, 0, ee_shift)), formed in
    longdouble and rounded once."""
    from qtos_amd import joints
    R = joints.rotation(np.asarray(euler, F64), LD)
    out = np.zeros((4, 3))
    for e in range(4):
        p = np.asarray(rob.hip[e], F64).astype(LD) + mirrored(r, e, rob)
        p[2] -= LD(EE_SHIFT)
        out[e] = (np.asarray(com, F64).astype(LD) + R @ p).astype(F64)
    return out


def step(v, k):
    """v moved k units in the last place away from zero (k < 0: towards it)."""
    v = F64(v)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, np.copysign(np.inf, v) if k > 0 else F64(0.0))
    return v


def margins(feet, rob, dtype=F64):
    """(c3 [4], h2 [4]) of the statement for feet at identity attitude with the CoM at the origin."""
    from qtos_amd import joints
    zero = np.zeros(3)
    out = [joints.ik_margins(e, joints.base_frame(zero, zero, feet[e], EE_SHIFT, dtype=dtype)[0], rob, dtype) for e in range(4)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def stepped(feet, axis, ks):
    """The feet with coordinate `axis` of foot e moved ks[e] units in the last place."""
    out = np.array(feet, F64)
    for e in range(4):
        out[e, axis] = step(out[e, axis], ks[e])
    return out


def probes():
    """The table of the SOLO12 launch, in order (at most 64: one window each)."""
    if "probes" in _cache:
        return _cache["probes"]
    rob = robot("solo12")
    reach = rob.l_upper + rob.l_lower
    P = []

    def add(name, cls, r, **kw):
        P.append(Probe(name, cls, world_feet(r, rob), **kw))
        return P[-1]

    down = world_feet((0.0, 1.0, -reach), rob)
    for k in range(-STEPS, STEPS + 1):
        P.append(Probe("stretch_down%+d" % k, "stretch_down", stepped(down, 2, [k] * 4)))
    EXACT["c3 == 1"] = False
    for ky in range(-STEPS, STEPS + 1):
        for kz in range(-STEPS, STEPS + 1):
            f = stepped(stepped(down, 1, [ky] * 4), 2, [kz] * 4)
            if not EXACT["c3 == 1"] and (margins(f, rob)[0] == 1).all():
                EXACT["c3 == 1"] = True
                P.append(Probe("stretch_exact", "stretch_exact", f))
    add("stretch_x+", "stretch_x", (reach, 1.0, 0.0))
    add("stretch_x-", "stretch_x", (-reach, 1.0, 0.0))
    add("beyond", "beyond", (0.0, 1.0, -1.5 * reach))
    for k in (4, 8, 12):
        rho = LD(rob.l_upper) * np.sqrt(LD(4) - 2 * LD(10) ** -k)
        add("near_straight_%d" % k, "near_straight", (0.0, 1.0, -rho))
    for k in (3, 8):
        add("near_fold_%d" % k, "near_fold", (0.0, 1.0, -LD(10) ** -k))
    add("near_fold_0", "near_fold", (0.0, 1.0, 0.0))
    add("inside", "inside", (0.1, 0.5, 0.0))
    add("inside_x0", "inside", (0.0, 0.5, 0.0))               # r_x = 0 and h = 0: atan2(-0, 0), where atan(-r_x / h) has no value
    edge = world_feet((0.1, 1.0, 0.0), rob)
    sides = {"-": [None] * 4, "+": [None] * 4, "=0": [None] * 4}
    for k in sorted(range(-STEPS, STEPS + 1), key=abs):
        h2 = margins(stepped(edge, 1, [k] * 4), rob)[1]
        for e in range(4):
            key = "-" if h2[e] < 0 else ("+" if h2[e] > 0 else "=0")
            if sides[key][e] is None:
                sides[key][e] = k
    assert None not in sides["-"] and None not in sides["+"]
    EXACT["h2 == 0"] = None not in sides["=0"]
    for key in ("-", "+") + (("=0",) if EXACT["h2 == 0"] else ()):
        P.append(Probe("inside_h2" + key, "inside", stepped(edge, 1, sides[key])))
    add("quadrant_above", "quadrants", (0.05, 1.0, 0.2))
    add("quadrant_level_out", "quadrants", (0.05, 0.0, 0.0, 0.25))
    add("quadrant_level_in", "quadrants", (-0.05, 0.0, 0.0, -0.2))
    add("quadrant_behind_under", "quadrants", (-0.1, 0.0, -0.24))
    for i, eul in enumerate(ATTITUDES):
        P.append(Probe("attitude_%d" % i, "attitudes", world_feet((0.0, 1.0, -0.24), rob, ATTITUDE_COM, eul), ATTITUDE_COM, eul))
    by_name = {p.name: p for p in P}
    for src in ("near_straight_4", "near_straight_8", "quadrant_above", "attitude_5"):
        for j, (cv, er) in enumerate(VELOCITIES):
            P.append(by_name[src].moved("moving_%s_%d" % (src, j), "moving", cv, er))
    nominal = world_feet((0.0, 1.0, -0.24), rob)
    P.append(Probe("nominal", "nominal", nominal))
    for tag, bad in (("nan", np.nan), ("inf", np.inf)):
        for d in range(3):
            f = nominal.copy()
            f[1, d] = bad
            P.append(Probe("nonfinite_foot1_%s_%s" % ("xyz"[d], tag), "nonfinite", f, bad_q=(1,)))
        P.append(Probe("nonfinite_com_%s" % tag, "nonfinite", nominal, com=(bad, 0.0, 0.0), bad_q=(0, 1, 2, 3)))
        P.append(Probe("nonfinite_euler_%s" % tag, "nonfinite", nominal, euler=(0.0, bad, 0.0), bad_q=(0, 1, 2, 3)))
        g = FORCES.copy()
        g[2, 2] = bad
        P.append(Probe("nonfinite_force2_%s" % tag, "nonfinite", nominal, forces=g, bad_tau=(2,)))
    assert len(P) <= 64 and len({p.name for p in P}) == len(P)
    _cache["probes"] = P
    return P


def fit_probe():
    """The static pose plan of the force kernels' torque test: the nominal stance under a tilted attitude with the weight shared
    by four vertical forces -- a plan in equilibrium, which the fit leaves nearly alone and the QP does not limit."""
    c = cfg()
    com, euler = ATTITUDE_COM, (0.1, -0.15, 0.7)
    f = np.tile([0.0, 0.0, c.mass * c.gravity / 4], (4, 1))
    return Probe("equilibrium", "fit", world_feet((0.0, 1.0, -0.24), robot("solo12"), com, euler), com, euler, forces=f)


def fold_probes():
    """The table of the launch with unequal links."""
    if "fold" in _cache:
        return _cache["fold"]
    rob = robot("fold")
    P = [Probe("fold", "fold", world_feet((0.0, 1.0, -0.01), rob), robot_name="fold")]
    edge = world_feet((0.0, 1.0, -0.02), rob)
    for k in range(-STEPS, STEPS + 1, 2):                     # (a unit in the last place of the foot's z moves c3 by 1 / 40 of its own here)
        P.append(Probe("fold_edge%+d" % (FOLD_STEP * k), "fold_edge", stepped(edge, 2, [FOLD_STEP * k] * 4), robot_name="fold"))
    P.append(Probe("fold_clear", "fold_clear", world_feet((0.02, 1.0, -0.2), rob), robot_name="fold"))
    _cache["fold"] = P
    return P


class Statement:
    """What the statement says of a probe at row 0, in `dtype`: p_b, v_b, c3, h2 [4, ...], q, qd, tff [4, 3], the status word and
    R, straight from the pose (no spline in between)."""

    def __init__(self, probe, dtype):
        from qtos_amd import joints
        par = statement_params(probe.robot_name)
        self.p_b, self.v_b = np.zeros((4, 3), dtype), np.zeros((4, 3), dtype)
        self.c3, self.h2 = np.zeros(4, dtype), np.zeros(4, dtype)
        rows = np.zeros((1, 37), dtype)
        rows[0, 1:4], rows[0, 4:7], rows[0, 7:19] = probe.com, probe.euler, probe.feet.ravel()
        rows[0, 19:22], rows[0, 22:25], rows[0, 25:37] = probe.com_vel, probe.euler_rate, probe.forces.ravel()
        with np.errstate(all="ignore"):
            for e in range(4):
                p, v = joints.base_frame(probe.com, probe.euler, probe.feet[e], EE_SHIFT, probe.com_vel, probe.euler_rate, np.zeros(3), dtype)
                self.p_b[e], self.v_b[e] = p, v
                self.c3[e], self.h2[e] = joints.ik_margins(e, p, par, dtype)
            q, qd, tff, st = joints.joint_state(rows, np.zeros((1, 4, 3), dtype), par, dtype)
            self.R = joints.rotation(probe.euler, dtype)
        self.q, self.qd, self.tff, self.status = q.reshape(4, 3), qd.reshape(4, 3), tff.reshape(4, 3), int(st[0])

    def leg_bits(self, e):
        return (self.status >> e) & 0x1111

    def decided(self, e):
        """Whether leg e's three comparisons are further than MARGIN from their thresholds."""
        return bool(abs(self.c3[e] - 1) > MARGIN and abs(self.c3[e] + 1) > MARGIN and abs(self.h2[e]) > MARGIN)


def statement(probe, dtype):
    key = ("st", probe.name, np.dtype(dtype).name)
    if key not in _cache:
        _cache[key] = Statement(probe, dtype)
    return _cache[key]


def reachable_target(probe, e):
    """What the round trip of leg e is held to, in longdouble: p_b, or on REACH the foot of the straight leg that points at it
    -- the point of the reach sphere on the ray from the hip's pitch axis point (hip + Rx(q1) (0, d, 0)) to the target."""
    from qtos_amd import joints
    s = statement(probe, LD)
    if not s.leg_bits(e) & 1:
        return s.p_b[e]
    rob = robot(probe.robot_name)
    return joints.leg_fk(e, s.q[e], rob, LD)


def angle_rows():
    """[n, 3]: every triple of ANGLE_VALUES, then the float64 inverse kinematics' own angles of every finite leg of probes()."""
    if "angles" not in _cache:
        grid = np.array([(a, b, c) for a in ANGLE_VALUES for b in ANGLE_VALUES for c in ANGLE_VALUES])
        own = [statement(p, F64).q for p in probes() if p.finite]
        _cache["angles"] = (grid, np.array(own))
    return _cache["angles"]


def joint_table():
    """[n, 12] the angle probes as rows of four legs: a grid triple on every leg, then each finite probe's own four triples."""
    grid, own = angle_rows()
    return np.concatenate([np.tile(grid, (1, 4)), own.reshape(len(own), 12)])


def quat_of(euler):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll), float64."""
    e = np.asarray(euler, F64)
    sr, cr, sp_, cp, sy, cy = (f(e[..., i] / 2) for i in range(3) for f in (np.sin, np.cos))
    return np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], -1)


def quat_probes():
    """name -> (x, y, z, w)."""
    q = quat_of(TRACK_POSE[1])
    return {"unit": q, "norm3": 3.0 * q, "pitch+": np.array([0.0, 3.0, 0.0, 3.0]), "pitch-": np.array([0.0, -3.0, 0.0, 3.0]),
            "zero": np.zeros(4), "nan": np.array([q[0], np.nan, q[2], q[3]]), "inf": np.array([q[0], q[1], np.inf, q[3]])}


def chain_world(com, R, q12, dtype=LD):
    """The four feet in the world by the URDF's chain: com + R (chain(e, q_e) - (0, 0, ee_shift)), [n, 12]."""
    q12 = np.asarray(q12).reshape(-1, 12)
    out = np.zeros((len(q12), 12), dtype)
    for e in range(4):
        p, _ = jc.chain(e, q12[:, 3 * e:3 * e + 3], dtype)
        p = p.copy()
        p[:, 2] -= dtype(EE_SHIFT)
        out[:, 3 * e:3 * e + 3] = np.asarray(com).astype(dtype) + np.einsum("...ij,nj->ni" if np.ndim(R) == 2 else "nij,nj->ni", R, p)
    return out


def gate(floor, bound):
    return min(max(8.0 * float(floor), float(bound)), CAP)


def angle_gate(q3_ld):
    return min(U * (128 + 140 / max(abs(float(np.sin(q3_ld))), 1e-300)), CAP)


def same_numbers(a, b):
    """Bit for bit where finite; a NaN where a NaN is, an infinity of the same sign where one is."""
    a, b = np.ascontiguousarray(a, F64), np.ascontiguousarray(b, F64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(np.where(na, 0.0, a).view(np.int64), np.where(nb, 0.0, b).view(np.int64))


def record(name, entry):
    print("leg accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_LEG_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
