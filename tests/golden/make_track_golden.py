#!/usr/bin/env python3
"""Generate tests/golden/track.npz: what the reference's Tracking class records, as data.

Runs ONLY where the reference is checked out (its root: argv[1] or the environment variable QTOS_REFERENCE; its QTOS package is
imported with a `pybullet` stub as make_joint_golden.py does, and needs matplotlib, pandas and scipy); the test-suite uses the
committed output.  No reference source text is copied: only data.

The reference's QTOS.tracking and QTOS.utils are imported from the reference's directory; the runs then work in a temporary
directory with a logs/ folder, because Tracking.__init__ opens ./logs/experiment_data.out for writing.  The stand-in robot has
only a traj_vec attribute, the cfg is {"track": False, "track_rate": 10**9}: no plot is ever made.

  run A   calls 1 .. 700 with delay_tracking_itr at its own 500: ref_cmd = vec_to_cmd_pose(gait[k, 1:]) of row k = call - 1 of
          tests/golden/gait_pose.npz, traj_vec = that row's columns 1 .. 18 + a seeded normal perturbation of 1e-3
  run B   64 calls with delay_tracking_itr = 3

Per run X in (a, b): X_delay, X_traj_vec [calls, 18] (the perturbed inputs), X_error [recorded, 5] (the error lists CoM, FL, FR,
HL, HR), X_idx, X_total_com, X_total_feet [calls] (after every call).
"""
import os
import sys
import tempfile
import types

import numpy as np

REF = os.path.abspath(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("QTOS_REFERENCE", "reference"))
OUT = os.path.dirname(os.path.abspath(__file__))


class Robot:
    traj_vec = None


def run(tracking, rutils, pose, calls, delay, seed):
    rng = np.random.default_rng(seed)
    robot = Robot()
    T = tracking.Tracking(robot, calls, {"track": False, "track_rate": 10 ** 9})
    if delay is not None:
        T.delay_tracking_itr = delay
    vecs, idx, tc, tf = [], [], [], []
    for c in range(1, calls + 1):
        k = c - 1
        vec = pose[k] + 1e-3 * rng.standard_normal(18)
        vecs.append(vec.copy())
        robot.traj_vec = vec.copy()
        T.update(rutils.vec_to_cmd_pose(pose[k].copy()), k / 1000.0)
        idx.append(T.idx)
        tc.append(float(T.total_error_com_error))
        tf.append(float(T.total_error_feet_error))
    err = np.array([T.CoM_Pos["error"], T.FL_FOOT["error"], T.FR_FOOT["error"], T.HL_FOOT["error"], T.HR_FOOT["error"]], np.float64).T
    return dict(delay=np.int64(T.delay_tracking_itr), traj_vec=np.array(vecs), error=err.reshape(-1, 5), idx=np.array(idx, np.int64),
                total_com=np.array(tc), total_feet=np.array(tf))


def main():
    pose = np.load(os.path.join(OUT, "gait_pose.npz"))["pose"]
    sys.modules.setdefault("pybullet", types.ModuleType("pybullet"))
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    os.chdir(REF)
    try:
        from QTOS import tracking
        from QTOS import utils as rutils
        with tempfile.TemporaryDirectory() as tmp:
            os.makedirs(os.path.join(tmp, "logs"))
            os.chdir(tmp)
            a = run(tracking, rutils, pose, 700, None, 20241019)
            b = run(tracking, rutils, pose, 64, 3, 20241020)
            os.chdir(cwd)
    finally:
        os.chdir(cwd)
    assert a["delay"] == 500
    out = {}
    for name, r in (("a", a), ("b", b)):
        for k, v in r.items():
            out["%s_%s" % (name, k)] = v
    np.savez_compressed(os.path.join(OUT, "track.npz"), **out)


if __name__ == "__main__":
    sys.exit(main())
