"""What the joint tests share (tests/test_joints_cpu.py, tests/test_gpu_joints.py): the fixtures of tests/golden/joint_cmd.json and a
forward chain of the SOLO12 legs built from the fixture's joint origins and axes with generic transforms -- homogeneous matrices
and Rodrigues' rotation about the joint's axis, nothing of the closed form joints.py states -- with its geometric Jacobian
(axis x lever).  The number type is a parameter."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LEGS = ("FL", "FR", "HL", "HR")
_cache = {}


def fixture():
    if "fx" not in _cache:
        _cache["fx"] = json.load(open(os.path.join(GOLDEN, "joint_cmd.json")))
    return _cache["fx"]


def gait_pose():
    """Columns 1 .. 18 (CoM, Euler angles, feet) of all 5001 rows of the reference's test/data/traj/gait.csv."""
    if "pose" not in _cache:
        _cache["pose"] = np.load(os.path.join(GOLDEN, "gait_pose.npz"))["pose"]
    return _cache["pose"]


def _fixed(j, dtype):
    """The 4 x 4 transform of a joint's origin: translation xyz, rotation rpy (Rz Ry Rx, the URDF's convention)."""
    r, p, y = (dtype(v) for v in j["rpy"])
    Rx = np.array([[1, 0, 0], [0, np.cos(r), -np.sin(r)], [0, np.sin(r), np.cos(r)]], dtype)
    Ry = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]], dtype)
    Rz = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]], dtype)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = Rz @ Ry @ Rx
    T[:3, 3] = np.array(j["xyz"], np.float64).astype(dtype)
    return T


def _rodrigues(axis, ang, dtype):
    """[n, 4, 4]: rotation by ang [n] about the unit vector axis."""
    a = np.array(axis, np.float64).astype(dtype)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype)
    c, s = np.cos(ang)[:, None, None], np.sin(ang)[:, None, None]
    T = np.zeros((len(ang), 4, 4), dtype)
    T[:, :3, :3] = c * np.eye(3, dtype=dtype) + s * K + (1 - c) * np.outer(a, a)
    T[:, 3, 3] = 1
    return T


def chain(leg, q, dtype=np.longdouble):
    """Leg `leg` at the joint angles q [n, 3]: (foot [n, 3], J_geo [n, 3, 3]) in the base frame, column j of J_geo the joint's axis
    crossed with the lever from the joint to the foot."""
    urdf = fixture()["urdf"]
    q = np.asarray(q).astype(dtype).reshape(-1, 3)
    T = np.broadcast_to(np.eye(4, dtype=dtype), (len(q), 4, 4))
    axes, origins = [], []
    for j, name in enumerate(("HAA", "HFE", "KFE")):
        jt = urdf["%s_%s" % (LEGS[leg], name)]
        assert jt["type"] == "revolute"
        T = T @ _fixed(jt, dtype)
        axes.append(T[:, :3, :3] @ np.array(jt["axis"], np.float64).astype(dtype))
        origins.append(T[:, :3, 3])
        T = T @ _rodrigues(jt["axis"], q[:, j], dtype)
    ankle = urdf["%s_ANKLE" % LEGS[leg]]
    assert ankle["type"] == "fixed"
    T = T @ _fixed(ankle, dtype)
    foot = T[:, :3, 3]
    J = np.stack([np.cross(axes[j], foot - origins[j]) for j in range(3)], -1)
    return foot, J


def body_rate(euler, euler_rate, dtype=np.longdouble):
    """Angular velocity in the base frame of the pose R = Rz(yaw) Ry(pitch) Rx(roll) with the Euler rates given."""
    e, w = np.asarray(euler).astype(dtype), np.asarray(euler_rate).astype(dtype)
    sa, ca, sb, cb = np.sin(e[..., 0]), np.cos(e[..., 0]), np.sin(e[..., 1]), np.cos(e[..., 1])
    return np.stack([w[..., 0] - w[..., 2] * sb, w[..., 1] * ca + w[..., 2] * cb * sa, w[..., 2] * cb * ca - w[..., 1] * sa], -1)
