#!/usr/bin/env python3
"""Generate tests/golden/joint_cmd.json and gait_pose.npz: what the reference's consumer layer gives, as data.

Runs ONLY where the reference is checked out (its root: argv[1] or the environment variable QTOS_REFERENCE; its QTOS package is
imported with a `pybullet` stub as make_golden.py does); the test-suite uses the committed outputs.  No reference source text
is copied: only data.

  urdf            the twelve joint origins and axes (and the four fixed ankle origins) parsed from data/urdf/solo12.urdf
  towr_transform  QTOS/utils.py towr_transform's feet for rows 0, 25, .., 5000 of test/data/traj/gait.csv, with a stand-in robot
                  at the identity pose (CoM_states() returns list zeros, so transformation_mtx takes its Euler branch)
  motor           MotorModel outputs for seeded inputs that clip on both sides
  q_init          of data/config/solo12.yml
  gait_pose.npz   columns 1 .. 18 (CoM, Euler angles, feet) of all 5001 rows of gait.csv
"""
import json
import os
import re
import sys
import types
import xml.etree.ElementTree as ET

import numpy as np

REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("QTOS_REFERENCE", "reference"))
OUT = os.path.dirname(os.path.abspath(__file__))
EE = ("FL_FOOT", "FR_FOOT", "HL_FOOT", "HR_FOOT")


def urdf_fixture():
    root = ET.parse(os.path.join(REF, "data/urdf/solo12.urdf")).getroot()
    joints = {}
    for j in root.findall("joint"):
        name = j.get("name")
        if not re.match(r"^(FL|FR|HL|HR)_(HAA|HFE|KFE|ANKLE)$", name):
            continue
        axis = j.find("axis")
        joints[name] = {
            "type": j.get("type"), "parent": j.find("parent").get("link"), "child": j.find("child").get("link"),
            "xyz": [float(v) for v in j.find("origin").get("xyz").split()],
            "rpy": [float(v) for v in j.find("origin").get("rpy").split()],
            "axis": None if axis is None else [float(v) for v in axis.get("xyz").split()],
        }
    assert len(joints) == 16
    return joints


def towr_transform_fixture(gait):
    sys.modules.setdefault("pybullet", types.ModuleType("pybullet"))
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from QTOS import utils as rutils

        class Robot:
            def CoM_states(self):
                return {"linkWorldPosition": [0.0, 0.0, 0.0], "linkWorldOrientation": [0.0, 0.0, 0.0]}
        idx = list(range(0, 5001, 25))
        feet = []
        for k in idx:
            r = gait[k]
            traj = {"COM": np.array(r[1:7])}
            for e, name in enumerate(EE):
                traj[name] = {"P": np.array(r[7 + 3 * e:10 + 3 * e]), "D": np.zeros(3)}
            out = rutils.towr_transform(Robot(), traj, towr=True, ee_shift=0.015)
            feet.append([[float(v) for v in out[name]["P"]] for name in EE])
        return {"rows": idx, "ee_shift": 0.015, "feet": feet}
    finally:
        os.chdir(cwd)


def motor_fixture():
    sys.modules.setdefault("pybullet", types.ModuleType("pybullet"))
    sys.path.insert(0, REF)
    from QTOS.robot import robot_motor as rm
    rng = np.random.default_rng(20240917)
    n = 16
    q, q_mes = rng.uniform(-1.5, 1.5, (n, 12)), rng.uniform(-1.5, 1.5, (n, 12))
    qd, qd_mes = rng.uniform(-8.0, 8.0, (n, 12)), rng.uniform(-8.0, 8.0, (n, 12))
    q_mes[: n // 2] = q[: n // 2] + rng.uniform(-0.2, 0.2, (n // 2, 12))     # (half the rows near the command: not every torque clips)
    tff = rng.uniform(-4.0, 4.0, (n, 12))
    cases = []
    default_limit = float(rm.MOTOR.OBSERVED_TORQUE_LIMIT)
    for scales in ((1.0, 1.0, 1.0), (2.0, 1.5, 0.5)):
        for limit in (8.0, None):
            rm.MOTOR.OBSERVED_TORQUE_LIMIT = default_limit
            m = rm.MotorModel(20, 0.08, scales[0], scales[1], scales[2], toq_max=limit)
            lim = float(rm.MOTOR.OBSERVED_TORQUE_LIMIT)
            ff = np.array([m.convert_to_torque_ff(q[i], q_mes[i], qd_mes[i], qd[i], tff[i]) for i in range(n)])
            pd = np.array([m.convert_to_torque(q[i], q_mes[i], qd_mes[i], qd[i]) for i in range(n)])
            for name, t in (("ff", ff), ("pd", pd)):
                assert (t == lim).any() and (t == -lim).any() and (np.abs(t) < lim).any()
            cases.append({"kp": 20, "kd": 0.08, "scales": list(scales), "tau_max": lim, "kp_vec": m._kp.tolist(), "kd_vec": m._kd.tolist(),
                          "tau_ff": ff.tolist(), "tau_pd": pd.tolist()})
    rm.MOTOR.OBSERVED_TORQUE_LIMIT = default_limit
    return {"q": q.tolist(), "q_mes": q_mes.tolist(), "qd": qd.tolist(), "qd_mes": qd_mes.tolist(), "tau_ff_in": tff.tolist(),
            "default_limit": default_limit, "cases": cases}


def q_init():
    for ln in open(os.path.join(REF, "data/config/solo12.yml")):
        m = re.match(r"\s*q_init\s*:\s*\[(.*)\]", ln)
        if m:
            return [float(v) for v in m.group(1).split(",")]
    raise AssertionError("no q_init")


def main():
    gait = np.loadtxt(os.path.join(REF, "test/data/traj/gait.csv"), delimiter=",")
    assert gait.shape == (5001, 37)
    out = {"urdf": urdf_fixture(), "towr_transform": towr_transform_fixture(gait), "motor": motor_fixture(), "q_init": q_init()}
    json.dump(out, open(os.path.join(OUT, "joint_cmd.json"), "w"))
    np.savez_compressed(os.path.join(OUT, "gait_pose.npz"), pose=gait[:, 1:19])


if __name__ == "__main__":
    sys.exit(main())
