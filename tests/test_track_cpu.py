"""The tracking rule in numpy (qtos_amd/tracking.py, what k_track is held to) against the reference's data: what its Tracking class
records over two runs (tests/golden/track.npz, tests/golden/make_track_golden.py), the URDF chain of tests/joint_chain.py, the
round trip through joints.joint_rows, the quaternion mode, the ring form and the carried accumulators.

The error gate against the reference's np.linalg.norm is 2 units in the last place: on 50 000 random 3-vectors the explicit
formula sqrt((d0 d0 + d1 d1) + d2 d2) and np.linalg.norm differed in 5326 cases, every one by exactly one unit."""
import os

import numpy as np
import pytest

import joint_chain as jc
from conftest import GOLDEN, load_gv

from oracle import splines as sp
from qtos_amd import joints as J
from qtos_amd import tracking as T
from qtos_amd.config import PlannerConfig

LD, F64 = np.longdouble, np.float64
HZ = 200.0


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "track.npz"))


@pytest.fixture(scope="module")
def walk():
    """The golden walk: (layout, nodes)."""
    return sp.layout(PlannerConfig.reference_compat()), load_gv("gv1")["x"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def literal_reference(delay, calls):
    """Tracking.update's branch structure restated: the calls (1-based) that reach the recording branch."""
    num, flag, out = 0, False, []
    for _ in range(calls):
        num += 1
        if num < delay and not flag:
            pass
        elif num > delay and not flag:
            flag = True
        else:
            out.append(num)
    return out


@pytest.mark.parametrize("run,calls", [("a", 700), ("b", 64)])
def test_fixture_of_the_reference_class(golden, run, calls):
    delay = int(golden[run + "_delay"])
    vec, err_ref, idx = golden[run + "_traj_vec"], golden[run + "_error"], golden[run + "_idx"]
    assert delay == dict(a=500, b=3)[run] and vec.shape == (calls, 18)
    c = np.arange(1, calls + 1)
    rec = T.recorded(c, delay, "reference")
    assert np.array_equal(np.cumsum(rec), idx) and rec.sum() == len(err_ref)          # which calls were recorded, and idx after each
    assert c[rec][:3].tolist() == [delay, delay + 2, delay + 3]
    # the statement's errors against np.linalg.norm's
    ref_rows = np.concatenate([np.zeros((calls, 1)), jc.gait_pose()[:calls]], 1)
    err = T.errors(ref_rows, vec)
    assert err.dtype == F64 and err.shape == (calls, 5)
    ulp = np.abs(err[rec] - err_ref) / np.spacing(err_ref)
    print("track fixture %s: errors within %.0f units in the last place of np.linalg.norm (%d of %d differ)"
          % (run, ulp.max(), int((ulp > 0).sum()), ulp.size))
    assert ulp.max() <= 2
    # fed the fixture's own error values, the running totals are the reference's after every call, to the bit
    fed = np.zeros((calls, 5))
    fed[rec] = err_ref
    p = T.TrackParams(delay=delay)
    flags, totals, count, total = T.accumulate(fed, (0, 0), (0.0, 0.0), p)
    assert np.array_equal(flags, rec) and count == (calls, int(idx[-1]))
    assert np.array_equal(bits(totals[:, 0]), bits(golden[run + "_total_com"]))
    assert np.array_equal(bits(totals[:, 1]), bits(golden[run + "_total_feet"]))
    assert total == (golden[run + "_total_com"][-1], golden[run + "_total_feet"][-1])


@pytest.mark.parametrize("delay", [0, 1, 2, 3, 500])
def test_delay_rules(delay):
    c = np.arange(1, 601)
    assert c[T.recorded(c, delay, "reference")].tolist() == literal_reference(delay, 600)
    assert c[T.recorded(c, delay, "clean")].tolist() == [k for k in range(1, 601) if k > delay]
    assert bool(T.recorded(delay + 1, delay, "clean")) and not bool(T.recorded(delay + 1, delay, "reference"))
    with pytest.raises(ValueError):
        T.recorded(c, delay, "other")


def test_delay_of_the_reference_as_the_issue_lists_it():
    assert literal_reference(500, 503) == [500, 502, 503]
    assert literal_reference(3, 6) == [3, 5, 6]
    assert literal_reference(0, 3) == [2, 3]


def world(com, euler, p, dtype):
    """A base-frame point in the world through joint_chain's generic transform of an origin (xyz, rpy)."""
    out = np.zeros((len(p), 3), dtype)
    for i in range(len(p)):
        Tm = jc._fixed(dict(xyz=[float(v) for v in com[i]], rpy=[float(v) for v in euler[i]]), dtype)
        out[i] = Tm[:3, :3] @ p[i] + Tm[:3, 3]
    return out


def test_feet_are_the_urdf_chain_in_the_world():
    rng = np.random.default_rng(31)
    n = 40
    com, euler = rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-0.6, 0.6, (n, 3))
    q = rng.uniform(-1.2, 1.2, (n, 12))
    meas = np.concatenate([com, euler, q], 1)
    for dt, gate in ((LD, 1e-17), (F64, 4e-15)):
        pose = T.measured_pose(meas, T.TrackParams(ee_shift=0.0), dt)
        assert pose.dtype == dt and pose.shape == (n, 18)
        assert np.array_equal(pose[:, :6], meas[:, :6].astype(dt))                      # CoM and Euler columns are copied through
        worst = 0.0
        for e in range(4):
            foot, _ = jc.chain(e, q[:, 3 * e:3 * e + 3], LD)
            worst = max(worst, float(np.abs(pose[:, 6 + 3 * e:9 + 3 * e].astype(LD) - world(com, euler, foot, LD)).max()))
        print("feet against the URDF chain, %s: %.2e m" % (dt.__name__, worst))
        assert worst <= gate
    # ee_shift lowers the foot along the base's z axis
    a, b = T.measured_pose(meas, T.TrackParams(ee_shift=0.0), LD), T.measured_pose(meas, T.TrackParams(ee_shift=0.015), LD)
    R = J.rotation(euler, LD)
    for e in range(4):
        assert float(np.abs((a - b)[:, 6 + 3 * e:9 + 3 * e] - LD(0.015) * R[:, :, 2]).max()) <= 1e-18


def test_round_trip_through_the_joint_rows(walk):
    """A robot on its commanded angles and planned pose: no error on rows without a status bit; a leg beyond its reach is straight
    and its foot misses the plan by the distance the inverse kinematics could not cover."""
    L, x = walk
    n = 1001
    jp = J.JointParams()
    rows, status = J.joint_rows(L, x, 0.0, HZ, 0, n, jp, dtype=LD)
    plan = T.plan_positions(L, x, 0.0, HZ, 0, n, LD)
    meas = np.concatenate([plan[:, 1:7], rows[:, 1:13]], 1)
    out, st, count, total = T.track_rows(L, x, 0.0, HZ, 0, n, meas, T.TrackParams(delay=0, rule="clean"), dtype=LD)
    assert out.dtype == LD and out.shape == (n, 26) and (st == T.RECORDED).all() and count == (n, n)
    assert np.array_equal(out[:, 0], rows[:, 0]) and np.array_equal(out[:, 1:7], plan[:, 1:7])
    clean = status == 0
    assert 0 < clean.sum() < n
    print("round trip: %.2e m on %d rows without a status bit" % (float(out[clean, 19:24].max()), int(clean.sum())))
    assert float(out[clean, 19:24].max()) < 1e-15 and float(out[:, 19].max()) == 0
    Ltot = LD(jp.l_upper) + LD(jp.l_lower)
    seen = 0
    for e in range(4):
        r = ((status >> e) & 0x111) == 1                                                # reach, no fold, not inside
        assert ((status >> e) & 0x110 == 0).all()
        p_b, _ = J.base_frame(plan[:, 1:4], plan[:, 4:7], plan[:, 7 + 3 * e:10 + 3 * e], jp.ee_shift, dtype=LD)
        q = rows[:, 1 + 3 * e:4 + 3 * e]
        down, _ = jc.chain(e, np.stack([q[r, 0], 0 * q[r, 1], 0 * q[r, 2]], 1), LD)
        up, _ = jc.chain(e, np.stack([q[r, 0], 0 * q[r, 1] + LD(np.pi), 0 * q[r, 2]], 1), LD)
        ray = p_b[r] - (down + up) / 2
        short = np.sqrt((ray * ray).sum(1)) - Ltot
        assert (short > 0).all()
        assert float(np.abs(out[r, 20 + e] - short).max()) < 1e-15
        assert float(out[~r, 20 + e].max()) < 1e-15
        seen += int(r.sum())
    assert seen > 0
    assert total[0] == 0.0 and total[1] > 0 and float(out[-1, 25]) == total[1]


def quat_of(euler, dtype):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll): the product of three axis quaternions."""
    e = np.asarray(euler).astype(dtype)
    sr, cr, sp_, cp, sy, cy = (f(e[:, i] / 2) for i in range(3) for f in (np.sin, np.cos))
    return np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], 1)


def quat_rotate(q, v):
    """v turned by the unit quaternion q = (x, y, z, w): v + 2 w (u x v) + 2 u x (u x v)."""
    u, w = q[:, :3], q[:, 3:4]
    c = np.cross(u, v)
    return v + 2 * w * c + 2 * np.cross(u, c)


def test_quaternion_mode():
    rng = np.random.default_rng(32)
    n = 60
    euler = np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-1.2, 1.2, n), rng.uniform(-3.0, 3.0, n)], 1)
    com, q = rng.uniform(-1.0, 1.0, (n, 3)), rng.uniform(-1.2, 1.2, (n, 12))
    quat = quat_of(euler, LD)
    quat = quat / np.sqrt((quat * quat).sum(1))[:, None]
    p = T.TrackParams(quaternion=True)
    meas = np.concatenate([com.astype(LD), quat, q.astype(LD)], 1)
    pose, st = T.measured_pose(meas, p, LD, with_status=True)
    assert (st == 0).all()
    # R of the Euler columns is R of the quaternion, column by column through the quaternion product
    R = J.rotation(pose[:, 3:6], LD)
    worst = 0.0
    for j in range(3):
        axis = np.zeros((n, 3), LD)
        axis[:, j] = 1
        worst = max(worst, float(np.abs(R[:, :, j] - quat_rotate(quat, axis)).max()))
    worst_q = float(np.abs(T.quat_rotation(quat, LD) - R).max())
    print("quaternion mode: R(euler_out) - R(quat) %.2e, against quat_rotation %.2e" % (worst, worst_q))
    assert worst <= 1e-17 and worst_q <= 1e-17
    assert float(np.abs(pose[:, 3:6] - euler).max()) <= 1e-15                            # (the angles the quaternions were made of)
    # the same rows as the Euler mode gives for those angles
    same = T.measured_pose(np.concatenate([com.astype(LD), pose[:, 3:6], q.astype(LD)], 1), T.TrackParams(), LD)
    assert float(np.abs(same - pose).max()) <= 1e-17
    # a quaternion that is not normalised: the same rows (a power of two: to the bit)
    for scale, gate in ((2.0, 0.0), (3.7, 1e-17)):
        scaled = meas.copy()
        scaled[:, 3:7] *= LD(scale)
        assert float(np.abs(T.measured_pose(scaled, p, LD) - pose).max()) <= gate
    with pytest.raises(ValueError):
        T.measured_pose(meas[:, :18], p, LD)
    # pitch = pi / 2: the clip acts
    for dt in (F64, LD):
        m = np.zeros((2, 19), dt)
        m[0, 3:7] = (0, 3, 0, 3)                                                      # (y = w; 3 / sqrt(18) squares to 1/2 or above in both types)
        m[1, 3:7] = (0, 0, 0, 1)
        g, st = T.measured_pose(m, p, dt, with_status=True)
        assert st.tolist() == [T.GIMBAL, 0] and abs(float(g[0, 4]) - np.pi / 2) < 1e-7 and float(g[1, 4]) == 0


def test_ring_carry_over_and_reached(walk):
    L, x = walk
    rng = np.random.default_rng(33)
    n, cap, t0 = 90, 64, 2.5
    jp = J.JointParams()
    rows, _ = J.joint_rows(L, x, t0, HZ, 300, n, jp, dtype=F64)
    plan = T.plan_positions(L, x, t0, HZ, 300, n, F64)
    meas = np.concatenate([plan[:, 1:7], rows[:, 1:13]], 1) + 1e-3 * rng.standard_normal((n, 18))
    goal_x = float(np.sort(meas[:, 0])[n // 2])
    for rule in T.RULES:
        p = T.TrackParams(delay=3, rule=rule)
        one, st, count, total = T.track_rows(L, x, t0, HZ, 300, n, meas, p, (0, 0), (0.0, 0.0), goal_x, F64)
        assert one.dtype == F64 and count == (n, n - 3) and total == (one[-1, 24], one[-1, 25])
        assert ((st & T.REACHED) != 0).tolist() == (meas[:, 0] >= goal_x).tolist() and 0 < ((st & T.REACHED) != 0).sum() < n
        assert ((st & T.RECORDED) != 0).tolist() == T.recorded(np.arange(1, n + 1), 3, rule).tolist()
        free = T.track_rows(L, x, t0, HZ, 300, n, meas, p, dtype=F64)[1]
        assert ((free & T.REACHED) == 0).all()                                          # without goal_x the bit is never set
        # the totals are float64 additions in program order
        tc = tf = 0.0
        for j in range(n):
            if st[j] & T.RECORDED:
                tc += float(one[j, 19])
                for e in range(4):
                    tf += float(one[j, 20 + e])
            assert one[j, 24] == tc and one[j, 25] == tf
        # two calls in a row with the accumulators carried over: one call over the concatenation, to the bit
        cut = 37
        a, sa, ca, ta = T.track_rows(L, x, t0, HZ, 300, cut, meas[:cut], p, (0, 0), (0.0, 0.0), goal_x, F64)
        b, sb, cb, tb = T.track_rows(L, x, t0, HZ, 300 + cut, n - cut, meas[cut:], p, ca, ta, goal_x, F64)
        assert np.array_equal(bits(np.concatenate([a, b])), bits(one)) and np.array_equal(np.concatenate([sa, sb]), st)
        assert cb == count and tb == total
        # the ring form: two appends, the second wraps
        ring_m, ring_o, ring_s = np.full((cap, 18), np.nan), np.full((cap, 26), -7.5), np.full(cap, -7, np.int32)
        cur, cnt, tot = 50, (0, 0), (0.0, 0.0)
        for first, m in ((0, cut), (cut, n - cut)):
            at = (cur + np.arange(m)) % cap
            ring_m[at] = meas[first:first + m]
            cnt, tot = T.track_ring(L, x, t0, HZ, 300 + first, m, ring_m, cur, p, ring_o, ring_s, cnt, tot, goal_x, F64)
            if first == 0:
                assert (ring_o[np.setdiff1d(np.arange(cap), at)] == -7.5).all()
            cur += m
        assert cnt == count and tot == total and cur - 50 > cap
        from qtos_amd.stitcher import ring_rows
        assert np.array_equal(bits(ring_rows(ring_o, cur)), bits(one[-cap:])) and np.array_equal(ring_rows(ring_s, cur), st[-cap:])
    # the ctypes mirror is read the same way
    from qtos_amd import capi
    same = T.track_rows(L, x, t0, HZ, 300, n, meas, capi.track_params(delay=3, rule="clean"), (0, 0), (0.0, 0.0), goal_x, F64)
    assert np.array_equal(bits(same[0]), bits(one)) and np.array_equal(same[1], st)
