"""The joint-command rule in numpy (qtos_amd/joints.py, what k_joint_rows is held to) against the reference's data: the URDF's joint
origins, towr_transform's feet, MotorModel's torques and all 5001 rows of the reference's canned plan gait.csv
(tests/golden/joint_cmd.json, gait_pose.npz; tests/golden/make_joint_golden.py).  The forward chain the inverse kinematics, the
Jacobian and the torques are checked with is tests/joint_chain.py: generic transforms from the fixture's origins and axes."""
import numpy as np
import pytest

import joint_chain as jc
from conftest import load_gv

from oracle import splines as sp
from qtos_amd import joints as J
from qtos_amd.config import PlannerConfig

LD, F64 = np.longdouble, np.float64
EE_SHIFT = 0.015
REACH_COUNTS = (76, 93, 99, 59)      # rows of gait.csv with the leg's target beyond its reach, and with any: 6.54 % of 5001
FLAGGED_ROWS = 327


def test_solo12_is_the_urdfs_leg():
    urdf = jc.fixture()["urdf"]
    for e, leg in enumerate(jc.LEGS):
        haa, hfe, kfe, ankle = (urdf["%s_%s" % (leg, n)] for n in ("HAA", "HFE", "KFE", "ANKLE"))
        assert haa["parent"] == "base_link" and ankle["child"] == leg + "_FOOT"
        assert haa["axis"] == [1, 0, 0] and hfe["axis"] == [0, 1, 0] and kfe["axis"] == [0, 1, 0]
        assert all(j["rpy"] == [0, 0, 0] for j in (haa, hfe, kfe, ankle))
        assert J.SOLO12.hip[e].tolist() == haa["xyz"]
        assert J.SOLO12.lateral[e] == np.sign(hfe["xyz"][1]) * (abs(hfe["xyz"][1]) + abs(kfe["xyz"][1]) + abs(ankle["xyz"][1]))
        assert hfe["xyz"][0] == hfe["xyz"][2] == kfe["xyz"][0] == ankle["xyz"][0] == 0
        assert J.SOLO12.l_upper == -kfe["xyz"][2] and J.SOLO12.l_lower == -ankle["xyz"][2]
    q_init = np.array(jc.fixture()["q_init"]).reshape(4, 3)
    assert (np.sign(q_init[:, 2]) == J.SOLO12.knee_sign).all()          # the branch of the reference's rest pose
    assert J.LEGS == jc.LEGS and J.JOINTS == ("HAA", "HFE", "KFE")


def test_base_frame_is_towr_transform():
    """Gate: 8 units of 2^-53 (|p_c|_1 + |p_f|_1) per coordinate -- the reference rounds R^T p_f and R^T p_c separately, each to
    half an ulp of a sum of three products bounded by the 1-norms (measured: 2.3 units)."""
    tt, pose = jc.fixture()["towr_transform"], jc.gait_pose()
    idx, feet = np.array(tt["rows"]), np.array(tt["feet"])
    assert idx.tolist() == list(range(0, 5001, 25)) and tt["ee_shift"] == EE_SHIFT
    worst = 0.0
    for e in range(4):
        com, foot = pose[idx, 0:3], pose[idx, 6 + 3 * e:9 + 3 * e]
        p_b, v_b = J.base_frame(com, pose[idx, 3:6], foot, EE_SHIFT, dtype=F64)
        assert v_b is None and p_b.dtype == F64
        unit = 2.0 ** -53 * (np.abs(com).sum(1) + np.abs(foot).sum(1))
        worst = max(worst, float((np.abs(p_b - feet[:, e]) / unit[:, None]).max()))
    print("base_frame against towr_transform: %.2f units" % worst)
    assert worst <= 8.0


@pytest.fixture(scope="module")
def gait_ik():
    """Per number type and leg: (p_b, q, status) of all rows of gait.csv."""
    pose = jc.gait_pose()
    out = {}
    for dt in (F64, LD):
        for e in range(4):
            p_b, _ = J.base_frame(pose[:, 0:3], pose[:, 3:6], pose[:, 6 + 3 * e:9 + 3 * e], EE_SHIFT, dtype=dt)
            q, st = J.leg_ik(e, p_b, dtype=dt)
            assert q.dtype == dt and st.dtype == np.int32
            out[dt, e] = (p_b, q, st)
    return out


def test_status_counts_of_the_reference_plan(gait_ik):
    """The reference's plans ask more of the leg than the URDF's 0.32 m: with ee_shift 0.015, 327 of the 5001 rows of gait.csv
    have a leg beyond reach (Bullet's iterative IK hides it)."""
    for dt in (F64, LD):
        st = np.stack([gait_ik[dt, e][2] for e in range(4)], 1)
        assert ((st & ~J.REACH) == 0).all()                      # no fold, no inside
        assert tuple(int(v) for v in (st != 0).sum(0)) == REACH_COUNTS
        assert int((st != 0).any(1).sum()) == FLAGGED_ROWS


def test_ik_round_trip_through_the_urdf_chain(gait_ik):
    """Rows without a status bit: the chain at the IK's angles stands on the target to 1e-15 m in float64 (5 ulp of the leg's
    length; measured 2e-16 and less); in longdouble to 1e-17 m (the lateral offset is the float64 sum of the URDF's three offsets,
    2e-18 off the sum the longdouble chain forms).  A reach-flagged leg is straight and its foot lies on the ray from the hip-plane origin
    to the target, at l_u + l_l."""
    flagged = np.zeros(5001, bool)
    for e in range(4):
        flagged |= gait_ik[F64, e][2] != 0
    assert flagged.sum() <= 0.1 * len(flagged)
    L = J.SOLO12.l_upper + J.SOLO12.l_lower
    for dt, gate in ((F64, 1e-15), (LD, 1e-17)):
        worst = 0.0
        for e in range(4):
            p_b, q, st = gait_ik[dt, e]
            foot, _ = jc.chain(e, q, dt)
            worst = max(worst, float(np.abs(foot - p_b)[~flagged].max()))
            r = st != 0
            assert (q[r, 2] == 0).all()
            # the hip-plane origin: a straight leg swung half a turn about the HFE ends opposite to where it began
            down, _ = jc.chain(e, np.stack([q[r, 0], 0 * q[r, 1], 0 * q[r, 2]], 1), dt)
            up, _ = jc.chain(e, np.stack([q[r, 0], 0 * q[r, 1] + dt(np.pi), 0 * q[r, 2]], 1), dt)
            origin = (down + up) / 2
            ray = p_b[r] - origin
            dist = np.sqrt((ray * ray).sum(1))
            assert (dist > dt(L)).all()
            on_ray = origin + ray * (dt(L) / dist)[:, None]
            assert float(np.abs(foot[r] - on_ray).max()) <= 8 * gate
        print("IK round trip, %s: %.2e m" % (dt.__name__, worst))
        assert worst <= gate


def test_fk_of_q_init_lands_where_the_chain_puts_it():
    q = np.array(jc.fixture()["q_init"]).reshape(4, 3)
    for e in range(4):
        for dt, gate in ((F64, 1e-15), (LD, 1e-17)):
            foot, Jg = jc.chain(e, q[e][None], dt)
            assert float(np.abs(J.leg_fk(e, q[e][None], dtype=dt) - foot).max()) <= gate
            assert float(np.abs(J.leg_jacobian(e, q[e][None], dtype=dt) - Jg).max()) <= gate
            back, st = J.leg_ik(e, foot, dtype=dt)          # q_init is on the branch the IK takes
            assert st[0] == 0 and float(np.abs(back - q[e]).max()) <= 100 * gate


@pytest.fixture(scope="module")
def plan_rows():
    """The golden walk sampled at 200 Hz, in both number types: (Cartesian rows, foot velocities) of joints.joint_rows."""
    cfg = PlannerConfig.reference_compat()
    L, x = sp.layout(cfg), load_gv("gv1")["x"]
    t = np.minimum(np.arange(1001) / 200.0, L.T)
    out = {}
    for dt in (F64, LD):
        rows = sp.sample_rows(L, x, 0.0, 200.0, 1001, dt)
        fv = np.stack([sp.eval_spline(L, 2 + e, x, t, 1, dt) for e in range(4)], 1)
        out[dt] = (rows, fv)
    return L, x, out


def test_rates_velocities_and_feed_forward(plan_rows):
    """qdot: |J_geo qdot - v_b| with the chain's geometric Jacobian; v_b a second way, R^T (pdot_f - pdot_c) - w_b x r_b;
    tau_ff = -J_geo^T f_b.  Gate of each: 8 x the float64 statement's own distance from its longdouble form, measured here, never
    above 1e-12.  The float64 statement and the longdouble one must both pass (the longdouble one by a factor of about 2^11)."""
    _, _, both = plan_rows
    params = J.JointParams()
    res = {dt: {} for dt in both}
    state = {}
    for dt, (rows, fv) in both.items():
        q, qd, tff, status = J.joint_state(rows, fv, params, dt)
        state[dt] = (q, qd, tff, status)
    assert (state[F64][3] == state[LD][3]).all()
    ok = np.stack([((state[LD][3] >> e) & 0x111) == 0 for e in range(4)], 1)
    assert ok.mean() > 0.9 and not ok.all()
    floor = dict(v_b=0.0, qdot=0.0, tau_ff=0.0)
    for e in range(4):
        sl = slice(3 * e, 3 * e + 3)
        rows, fv = both[LD]
        R = J.rotation(rows[:, 4:7], LD)
        r_b = np.einsum("nji,nj->ni", R, rows[:, 7 + 3 * e:10 + 3 * e] - rows[:, 1:4])
        v_ref = np.einsum("nji,nj->ni", R, fv[:, e] - rows[:, 19:22]) - np.cross(jc.body_rate(rows[:, 4:7], rows[:, 22:25], LD), r_b)
        f_b = np.einsum("nji,nj->ni", R, rows[:, 25 + 3 * e:28 + 3 * e])
        _, Jg = jc.chain(e, state[LD][0][:, sl], LD)           # the chain at the longdouble angles
        for dt, (rws, fvs) in both.items():
            q, qd, tff, _ = state[dt]
            _, v_b = J.base_frame(rws[:, 1:4], rws[:, 4:7], rws[:, 7 + 3 * e:10 + 3 * e], EE_SHIFT, rws[:, 19:22], rws[:, 22:25], fvs[:, e], dt)
            _, Jd = jc.chain(e, q[:, sl], LD)                 # the chain at the statement's own angles
            o = ok[:, e]
            res[dt]["v_b", e] = float(np.abs(v_b.astype(LD) - v_ref).max())
            res[dt]["qdot", e] = float(np.abs(np.einsum("nij,nj->ni", Jd, qd[:, sl].astype(LD)) - v_b.astype(LD))[o].max())
            res[dt]["tau_ff", e] = float(np.abs(tff[:, sl].astype(LD) + np.einsum("nji,nj->ni", Jd, f_b)).max())
            assert (qd[:, sl][~o] == 0).all()                 # a leg with a status bit stands still
        q64, qd64, t64, _ = state[F64]
        qL, qdL, tL, _ = state[LD]
        floor["v_b"] = max(floor["v_b"], res[F64]["v_b", e])
        floor["qdot"] = max(floor["qdot"], float(np.abs(np.einsum("nij,nj->ni", Jg, qd64[:, sl].astype(LD) - qdL[:, sl]))[ok[:, e]].max()))
        floor["tau_ff"] = max(floor["tau_ff"], float(np.abs(t64[:, sl].astype(LD) - tL[:, sl]).max()))
    for what, fl in floor.items():
        gate = min(8 * fl, 1e-12)
        for dt in both:
            worst = max(res[dt][what, e] for e in range(4))
            print("%s, %s: %.2e (floor %.2e, gate %.2e)" % (what, dt.__name__, worst, fl, gate))
            assert worst <= gate, (what, dt.__name__, worst, gate)


def test_motor_law_is_motormodels_to_the_bit():
    m = jc.fixture()["motor"]
    q, qd, qm, qdm, tff = (np.array(m[k]) for k in ("q", "qd", "q_mes", "qd_mes", "tau_ff_in"))
    assert m["default_limit"] == 3.0 and sorted({c["tau_max"] for c in m["cases"]}) == [3.0, 8.0]
    for c in m["cases"]:
        kp, kd = J.motor_gains(c["kp"], c["kd"], *c["scales"])
        assert (kp == np.array(c["kp_vec"])).all() and (kd == np.array(c["kd_vec"])).all()
        for key, ff in (("tau_ff", tff), ("tau_pd", None)):
            ref = np.array(c[key])
            assert (ref == c["tau_max"]).any() and (ref == -c["tau_max"]).any() and (np.abs(ref) < c["tau_max"]).any()
            assert (J.motor_torque(q, qd, ff, kp, kd, c["tau_max"], qm, qdm) == ref).all()
    # without measured values the PD terms are left out; tau_max <= 0 means no clip
    assert (J.motor_torque(q, qd, tff, kp, kd, 3.0) == np.clip(tff, -3.0, 3.0)).all()
    assert (J.motor_torque(q, qd, tff, kp, kd, 0.0, qm, qdm) == kp * (q - qm) + kd * (qd - qdm) + tff).all()
    p = J.JointParams()
    assert (p.kp == 20.0).all() and (p.kd == 0.08).all() and p.tau_max == 8.0 and p.ee_shift == EE_SHIFT     # data/config/solo12.yml


def test_joint_rows_layout(plan_rows):
    L, x, both = plan_rows
    params = J.JointParams()
    rows, fv = both[LD]
    out, status = J.joint_rows(L, x, 3.5, 200.0, 0, 1001, params, dtype=LD)
    q, qd, tff, st = J.joint_state(rows, fv, params, LD)
    assert out.shape == (1001, 37) and status.dtype == np.int32 and (status == st).all()
    assert (out[:, 0] == LD(3.5) + (np.arange(1001) / 200.0).astype(LD)).all()
    assert (out[:, 1:13] == q).all() and (out[:, 13:25] == qd).all() and (out[:, 25:37] == np.clip(tff, -8, 8)).all()
    part, st_part = J.joint_rows(L, x, 3.5, 200.0, 400, 7, params, dtype=LD)        # first_row: the same rows
    assert (part == out[400:407]).all() and (st_part == status[400:407]).all()
    qm = np.array(q[:7] + 0.3, F64)                                                   # a measured state: PD + feed-forward, clipped
    mes, _ = J.joint_rows(L, x, 3.5, 200.0, 400, 7, params, q_mes=qm, qd_mes=np.zeros((7, 12)), dtype=LD)
    expect = np.clip(20 * (out[400:407, 1:13] - qm) + LD(0.08) * out[400:407, 13:25] + tff[400:407], -8, 8)
    assert (mes[:, 25:37] == expect).all() and (np.abs(mes[:, 25:37]) == 8).any()
    from qtos_amd import capi                                                        # the ctypes mirror is read the same way
    same, _ = J.joint_rows(L, x, 3.5, 200.0, 400, 7, capi.joint_params(), dtype=LD)
    assert (same == part).all()
