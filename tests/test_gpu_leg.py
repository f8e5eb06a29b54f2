"""The three kernel copies of the SOLO12 leg chain on the MI355X (pytest -m gpu), at the edges of the leg's reach: k_joint_rows
(joint_leg: both instantiations), k_track (track_leg, track_pose: Euler and quaternion mode, both instantiations) and k_force_fit /
k_force_qp (fit_foot_out) on the probe table of tests/leg_cases.py, which states the probes, the pose plans and the derivation of
every gate.  One planner on the 464-variable transcription, one window per probe, every case one or two launches.

What is held.  Status: equal to the float64 statement's word at every identity-attitude probe, thresholds included and no margin
left out (both see the same bits of c3 and h^2); elsewhere equal to the longdouble statement's where c3 -+ 1 and h^2 are further
than 1e-12 from 0.  Angles: 256 u rad from the float64 statement at identity attitude, the angle gate of tests/test_gpu_joints.py from
the longdouble one elsewhere.  Round trip through the URDF's chain, rates and torques: leg_cases' gates.  A leg with a status bit
stands still, a straight leg has q3 = 0.  The motor law on these rows is joints.motor_torque to the bit.  Non-finite input: no
finite angle or rate out of a non-finite target, bit 12 + e, the other legs untouched (include/qtos_planner.h).  The same angles
through k_track's chain come back to the planned feet within 128 u m.

Measured on an MI355X: profiles/leg_accuracy.json.

Next to the full fold the round trips hold because of the rule's fold side (c3 < -1/2: h^2 as (r_y - d)(r_y + d) + r_z^2, the knee
from the half angle; joints.leg_ik).  Formed from c3 alone, kernel and float64 statement were 1.99e-11 m (near_fold_8) and
1.07e-9 m (near_fold_0) off the target, against a gate capped at 1e-12 m, and as far off the planned feet through k_track's chain.

Two checks are stated differently from the first plan for them, because what they rested on does not hold.  A static probe's
rows behind row 0 have the angles, torques and status of row 0 to the bit, but their rates are held to one another and not to
row 0: the kernels' evaluator leaves a velocity of 1e-30 m/s on a constant foot at t = T, and the chain multiplies it (by 3e17
on an unflagged leg at c3 == -1).  And k_force_fit's and k_force_qp's torques are compared to the bit where the QP does not limit
a row and its forces are the fit's to the bit: elsewhere the two kernels' forces differ by up to 2.7e-14 N
(tests/test_gpu_force_qp.py holds them to 1e-6 N), and each kernel's torques are held to its own forces."""
import numpy as np
import pytest

import joint_chain as jc
import leg_cases as lc
from leg_cases import CAP, F64, LD, U

pytestmark = pytest.mark.gpu
CLASSES = ("stretch_down", "stretch_x", "beyond", "near_straight", "near_fold", "inside", "quadrants", "attitudes", "moving", "nominal")
TRACK_HZ = 1000.0


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Rig:
    """The planner, the probes' nodes and what k_joint_rows makes of them: the one-wave tick (n_rows = 1) and the 512-lane tile
    (n_rows = 65), without measured state and clip (columns 25 .. 36 are tau_ff)."""

    def __init__(self):
        from qtos_amd import capi
        from qtos_amd.capi import Planner
        self.probes, self.folds = lc.probes(), lc.fold_probes()
        self.P = Planner(lc.cfg(), max_batch=64)
        self.L = lc.layout()
        assert self.P.n == self.L.n_vars == 464
        self.by = {p.name: i for i, p in enumerate(self.probes)}
        self.nodes = np.stack([p.nodes(self.L) for p in self.probes])
        self.fold_nodes = np.stack([p.nodes(self.L) for p in self.folds])
        self.t0 = np.zeros(len(self.probes))
        self.tick, self.tick_st = self.P.joint_rows(self.nodes, self.t0, capi.joint_params(hz=lc.HZ, n_rows=1, tau_max=0.0))
        self.tile, self.tile_st = self.P.joint_rows(self.nodes, self.t0, capi.joint_params(hz=lc.HZ, n_rows=lc.TILE_ROWS, tau_max=0.0))
        fold = lc.robot("fold")
        self.fold, self.fold_st = self.P.joint_rows(self.fold_nodes, np.zeros(len(self.folds)),
                                                    capi.joint_params(hz=lc.HZ, n_rows=1, tau_max=0.0, robot=fold))
        self.fold_tile, self.fold_tile_st = self.P.joint_rows(self.fold_nodes, np.zeros(len(self.folds)),
                                                              capi.joint_params(hz=lc.HZ, n_rows=lc.TILE_ROWS, tau_max=0.0, robot=fold))
        for a in (self.tick, self.tile, self.fold, self.fold_tile):
            a.setflags(write=False)

    def leg(self, i, e, rows=None):
        """(q, qd, tau_ff) [3] of leg e of probe i, and its four status bits."""
        r = (self.tick if rows is None else rows)[i, 0]
        return r[1 + 3 * e:4 + 3 * e], r[13 + 3 * e:16 + 3 * e], r[25 + 3 * e:28 + 3 * e]


_rig = {}


@pytest.fixture(scope="module")
def rig():
    _rig["rig"] = Rig()
    yield _rig["rig"]
    _rig.pop("rig").P.close()


def leg_bits(word, e):
    return (int(word) >> e) & 0x1111


def test_the_two_instantiations_agree_and_a_static_probe_is_every_row(rig):
    from qtos_amd import capi
    # a row behind row 0 through the one-wave kernel: the tile's row, to the bit
    last, last_st = rig.P.joint_rows(rig.nodes, rig.t0, capi.joint_params(hz=lc.HZ, first_row=lc.TILE_ROWS - 1, n_rows=1, tau_max=0.0))
    assert lc.same_numbers(last[:, 0, 1:], rig.tile[:, -1, 1:]) and np.array_equal(last_st[:, 0], rig.tile_st[:, -1])
    for rows, st, tile, tile_st, probes in ((rig.tick, rig.tick_st, rig.tile, rig.tile_st, rig.probes),
                                            (rig.fold, rig.fold_st, rig.fold_tile, rig.fold_tile_st, rig.folds)):
        assert rows.shape == (len(probes), 1, 37) and tile.shape == (len(probes), lc.TILE_ROWS, 37) and st.dtype == np.int32
        assert lc.same_numbers(rows[:, 0, 1:], tile[:, 0, 1:]) and np.array_equal(st[:, 0], tile_st[:, 0])
        for i, p in enumerate(probes):
            if p.static or not p.finite:
                # angles, torques and status: row 0 to the bit.  The rates: the rows behind row 0 (all at t = T, on two waves)
                # are one another to the bit and a leg with a status bit stands still in every row; they are not held to
                # row 0, whose foot velocity is another number (see leg_cases: the evaluator leaves 1e-30 m/s on a
                # constant foot at t = T, which an unflagged leg at c3 == -1, q3 = pi, sin q3 = 1.2e-16 turns into 8e-13 rad/s)
                for a, b in ((1, 13), (25, 37)):
                    assert lc.same_numbers(tile[i, :, a:b], np.broadcast_to(tile[i, 0, a:b], (lc.TILE_ROWS, 12))), p.name
                assert (tile_st[i] == tile_st[i, 0]).all(), p.name
                assert lc.same_numbers(tile[i, 1:, 13:25], np.broadcast_to(tile[i, 1, 13:25], (lc.TILE_ROWS - 1, 12))), p.name
                if p.finite:
                    flagged = np.repeat([leg_bits(st[i, 0], e) != 0 for e in range(4)], 3)
                    assert (tile[i, :, 13:25][:, flagged] == 0).all(), p.name
    seen = {}
    for i, p in enumerate(rig.probes + rig.folds):
        word = (rig.tick_st[i, 0] if i < len(rig.probes) else rig.fold_st[i - len(rig.probes), 0])
        print("leg probe [%s] %s: status per leg %s" % (p.cls, p.name, ["%#x" % leg_bits(word, e) for e in range(4)]))
        seen[p.cls] = seen.get(p.cls, 0) + 1
    assert set(seen) >= set(CLASSES) | {"nonfinite", "fold", "fold_edge", "fold_clear"}


def test_status_is_the_statements_at_every_threshold(rig):
    compared = 0
    for probes, st in ((rig.probes, rig.tick_st), (rig.folds, rig.fold_st)):
        for i, p in enumerate(probes):
            if not p.finite:
                continue
            assert int(st[i, 0]) & ~0xffff == 0
            if p.identity:
                assert int(st[i, 0]) == lc.statement(p, F64).status, (p.name, hex(int(st[i, 0])), hex(lc.statement(p, F64).status))
                compared += 4
            else:
                s = lc.statement(p, LD)
                for e in range(4):
                    if s.decided(e):
                        assert leg_bits(st[i, 0], e) == s.leg_bits(e), (p.name, e)
                        compared += 1
    assert compared >= 4 * (len(rig.probes) + len(rig.folds) - 12) - 8


def accuracy(rig, cls):
    """What the kernel's rows of a class are off by, against their gates: {probe: {quantity: (error, gate)}} (the worst leg)."""
    out = {}
    for i, p in enumerate(rig.probes):
        if p.cls != cls:
            continue
        s64, sld = lc.statement(p, F64), lc.statement(p, LD)
        v = dict(angle=(0.0, 1.0), fk=(0.0, 1.0), rate=(0.0, 1.0), torque=(0.0, 1.0))

        def worse(key, err, gate_):
            if err / gate_ >= v[key][0] / v[key][1]:
                v[key] = (float(err), float(gate_))
        for e in range(4):
            q, qd, tau = rig.leg(i, e)
            b = leg_bits(rig.tick_st[i, 0], e)
            assert np.isfinite(rig.tick[i, 0]).all() and not b & 0x1000, p.name
            if p.identity:
                worse("angle", np.abs(q - s64.q[e]).max(), lc.ANGLE_SAME_BITS)
            else:
                floor = float(np.abs(s64.q[e].astype(LD) - sld.q[e]).max())
                worse("angle", np.abs(q.astype(LD) - sld.q[e]).max(), min(max(8 * floor, lc.angle_gate(sld.q[e, 2])), CAP))
            foot, Jg = jc.chain(e, q, LD)
            foot64, J64 = jc.chain(e, s64.q[e], LD)
            if not b & 0x110:
                target = lc.reachable_target(p, e)
                worse("fk", np.abs(foot[0] - target).max(), lc.gate(np.abs(foot64[0] - target).max(), lc.FK_BOUND))
            if b:
                assert (qd == 0).all(), (p.name, e)
                if b & 1:
                    assert q[2] == 0, (p.name, e)
            else:
                floor = float(np.abs(J64[0] @ s64.qd[e].astype(LD) - sld.v_b[e]).max())
                res = float(np.abs(Jg[0] @ qd.astype(LD) - sld.v_b[e]).max())
                worse("rate", res, max(8 * floor, lc.RATE_BOUND * (1 + 0.5 * float(np.abs(qd).max()))))
            f_b = sld.R.T @ p.forces[e].astype(LD)
            floor = float(np.abs(s64.tff[e].astype(LD) + J64[0].T @ f_b).max())
            worse("torque", np.abs(tau.astype(LD) + Jg[0].T @ f_b).max(), lc.gate(floor, lc.TORQUE_BOUND * float(np.abs(p.forces[e]).sum())))
        out[p.name] = v
    return out


@pytest.mark.parametrize("cls", CLASSES)
def test_angles_rates_and_torques(rig, cls):
    acc = accuracy(rig, cls)
    assert acc
    lc.record("k_joint_rows %s" % cls, {n: {k: dict(error=e, gate=g) for k, (e, g) in v.items() if k != "fk"} for n, v in acc.items()})
    for name, v in acc.items():
        for key in ("angle", "rate", "torque"):
            assert v[key][0] <= v[key][1], (name, key, v[key])


@pytest.mark.parametrize("cls", CLASSES)
def test_round_trip(rig, cls):
    acc = accuracy(rig, cls)
    lc.record("k_joint_rows round trip %s" % cls, {n: dict(error=v["fk"][0], gate=v["fk"][1]) for n, v in acc.items()})
    for name, v in acc.items():
        assert v["fk"][0] <= v["fk"][1], (name, v["fk"])


def test_the_fold_bit(rig):
    """l_upper 0.17, l_lower 0.15: the FOLD bit, q3 = +-pi up to acos' 4 ulp, a standing leg; the threshold's probes as the
    float64 statement has them (test_status_is_the_statements_at_every_threshold); the angles at 256 u rad."""
    names = [p.name for p in rig.folds]
    i = names.index("fold")
    for e in range(4):
        q, qd, _ = rig.leg(i, e, rig.fold)
        assert leg_bits(rig.fold_st[i, 0], e) == 0x10 and (qd == 0).all()
        assert abs(abs(q[2]) - np.pi) <= 4 * np.spacing(np.pi) and np.sign(q[2]) == lc.robot("fold").knee_sign[e]
    flagged = {bool(leg_bits(rig.fold_st[names.index(n), 0], 0) & 0x10) for n in names if n.startswith("fold_edge")}
    assert flagged == {True, False}
    worst = 0.0
    for j, p in enumerate(rig.folds):
        s = lc.statement(p, F64)
        for e in range(4):
            worst = max(worst, float(np.abs(rig.leg(j, e, rig.fold)[0] - s.q[e]).max()))
    lc.record("k_joint_rows fold", dict(angle_error=worst, gate=lc.ANGLE_SAME_BITS))
    assert worst <= lc.ANGLE_SAME_BITS


def test_no_finite_number_comes_out_of_a_non_finite_target(rig):
    nominal = rig.by["nominal"]
    assert rig.tick_st[nominal, 0] == 0
    seen = 0
    for i, p in enumerate(rig.probes):
        if p.finite:
            continue
        seen += 1
        for rows, st in ((rig.tick, rig.tick_st), (rig.tile, rig.tile_st)):
            assert int(st[i, 0]) == lc.statement(p, F64).status, (p.name, hex(int(st[i, 0])))
            for e in range(4):
                q, qd, tau = rig.leg(i, e, rows)
                q0, qd0, tau0 = rig.leg(nominal, e, rows)
                b = leg_bits(st[i, 0], e)
                if e in p.bad_q:
                    assert np.isnan(q).all() and np.isnan(qd).all() and not np.isfinite(tau).any() and b & 0x1000, (p.name, e, q, qd, tau)
                else:
                    assert np.array_equal(bits(q), bits(q0)) and np.array_equal(bits(qd), bits(qd0)), (p.name, e)
                    if e in p.bad_tau:
                        assert not np.isfinite(tau).all() and b == 0x1000, (p.name, e)
                    else:
                        assert np.array_equal(bits(tau), bits(tau0)) and b == 0, (p.name, e)
    assert seen == 12


def test_motor_law_is_numpys_to_the_bit(rig):
    """With measured q and qdot, scaled gains and a clip, on the probes' rows: joints.motor_torque on the kernel's own q, qdot and
    tau_ff, bit for bit (a NaN where a NaN is)."""
    from qtos_amd import capi, joints
    rng = np.random.default_rng(7)
    B = len(rig.probes)
    q, qd, tff = rig.tick[:, 0, 1:13], rig.tick[:, 0, 13:25], rig.tick[:, 0, 25:37]
    q_mes = np.where(np.isfinite(q), q, 0.0) + rng.uniform(-0.3, 0.3, (B, 12))
    qd_mes = rng.uniform(-3.0, 3.0, (B, 12))
    hit = set()
    for scales, tau_max, ff in (((1.0, 1.0, 1.0), 8.0, True), ((2.0, 1.5, 0.5), 3.0, True), ((2.0, 1.5, 0.5), 3.0, False)):
        p = capi.joint_params(hz=lc.HZ, n_rows=1, hip_scale=scales[0], knee_scale=scales[1], ankle_scale=scales[2], tau_max=tau_max,
                              feed_forward=ff)
        kp, kd = joints.motor_gains(20.0, 0.08, *scales)
        got, st = rig.P.joint_rows(rig.nodes, rig.t0, p, q_mes=q_mes, qd_mes=qd_mes)
        assert lc.same_numbers(got[:, 0, 1:25], rig.tick[:, 0, 1:25])
        with np.errstate(invalid="ignore"):
            want = joints.motor_torque(q, qd, tff if ff else None, kp, kd, tau_max, q_mes, qd_mes)
        assert lc.same_numbers(got[:, 0, 25:37] + 0.0, want + 0.0), (scales, tau_max, ff)
        for i, pr in enumerate(rig.probes):                                   # without feed-forward a non-finite force reaches nothing
            want_st = int(rig.tick_st[i, 0]) if ff or not pr.bad_tau else 0
            assert int(st[i, 0]) == want_st, (pr.name, ff)
        hit |= {s for s, m in (("hi", got[:, 0, 25:37] == tau_max), ("lo", got[:, 0, 25:37] == -tau_max),
                               ("in", np.abs(got[:, 0, 25:37]) < tau_max)) if m.any()}
    assert hit == {"hi", "lo", "in"}


class Track:
    """k_track on the angle probes: the planned rows are a static pose plan (attitude_5), the measured rows carry TRACK_POSE and
    the joint table, then three non-finite rows.  One 512-lane launch over all rows and one one-wave launch over windows of 64."""

    def __init__(self, rig, quaternion):
        from qtos_amd import capi, tracking
        self.quat = quaternion
        table = lc.joint_table()
        nominal = lc.statement(rig.probes[rig.by["nominal"]], F64).q.ravel()
        com, euler = np.array(lc.TRACK_POSE[0]), np.array(lc.TRACK_POSE[1])
        if quaternion:
            Q = lc.quat_probes()
            head = np.stack([np.concatenate([com, Q["unit"] if j % 2 else Q["norm3"]]) for j in range(len(table))])
            self.special = list(Q)
            tail = np.stack([np.concatenate([com, Q[n], nominal]) for n in self.special])
        else:
            head = np.tile(np.concatenate([com, euler]), (len(table), 1))
            self.special = ["q nan", "com inf", "euler nan"]
            tail = np.tile(np.concatenate([com, euler, nominal]), (3, 1))
            tail[0, 6 + 4], tail[1, 0], tail[2, 3] = np.nan, np.inf, np.nan
        self.meas = np.concatenate([np.concatenate([head, table], 1), tail])
        self.n, self.n_regular = len(self.meas), len(table)
        self.nodes = rig.nodes[rig.by["attitude_5"]][None]
        self.rows, self.status, self.count, self.total = rig.P.track(
            self.nodes, 0.0, self.meas[None], capi.track_params(hz=TRACK_HZ, n_rows=self.n, delay=0, rule="clean", quaternion=quaternion))
        B = -(-self.n // 64)
        padded = np.zeros((B * 64, self.meas.shape[1]))
        padded[:self.n] = self.meas
        counts = np.minimum(64, self.n - 64 * np.arange(B)).astype(np.int32)
        self.wave, self.wave_st, _, _ = rig.P.track(np.repeat(self.nodes, B, axis=0), 0.0, padded.reshape(B, 64, -1),
                                                    capi.track_params(hz=TRACK_HZ, n_rows=64, delay=0, rule="clean", quaternion=quaternion),
                                                    first_row=(64 * np.arange(B)).astype(np.int32), n_rows=counts)
        par = tracking.TrackParams(delay=0, rule="clean", quaternion=quaternion)
        with np.errstate(all="ignore"):
            self.want = {dt: tracking.track_rows(rig.L, self.nodes[0], 0.0, TRACK_HZ, 0, self.n, self.meas, par, dtype=dt) for dt in (LD, F64)}


@pytest.mark.parametrize("quaternion", [False, True], ids=["euler", "quaternion"])
def test_track_chain_on_the_angle_probes(rig, quaternion):
    from qtos_amd import joints, tracking
    T = Track(rig, quaternion)
    assert T.n > 64 and T.rows.shape == (1, T.n, 26)
    got, (w_ld, st_ld, _, _), (w_64, st_64, cnt_64, tot_64) = T.rows[0], T.want[LD], T.want[F64]
    # the one-wave instantiation: the same pose columns and errors, to the bit
    flat = T.wave.reshape(-1, 26)[:T.n]
    assert lc.same_numbers(flat[:, 1:24], got[:, 1:24]) and np.array_equal(T.wave_st.reshape(-1)[:T.n] & 6, T.status[0] & 6)
    # status: exact; every column is finite exactly where the float64 statement's is
    assert np.array_equal(T.status[0], st_64)
    assert np.array_equal(np.isfinite(got), np.isfinite(w_64.astype(F64))), np.nonzero(np.isfinite(got) != np.isfinite(w_64.astype(F64)))
    assert tuple(T.count[0]) == cnt_64 and np.array_equal(np.isfinite(T.total[0]), np.isfinite(np.array(tot_64)))
    assert not np.isfinite(T.total[0]).all() and np.isfinite(got[:T.n_regular]).all()
    # the regular rows: feet against the longdouble statement and against the URDF's chain
    reg = slice(0, T.n_regular)
    floor = float(np.abs(w_64[reg, 7:19].astype(LD) - w_ld[reg, 7:19]).max())
    gate = lc.gate(floor, lc.FEET_BOUND)
    err = float(np.abs(got[reg, 7:19].astype(LD) - w_ld[reg, 7:19]).max())
    if quaternion:
        R = tracking.quat_rotation(T.meas[reg, 3:7], LD)
    else:
        R = joints.rotation(T.meas[reg, 3:6], LD)
    feet = lc.chain_world(T.meas[reg, 0:3], R, T.meas[reg, -12:], LD)
    err_chain = float(np.abs(got[reg, 7:19].astype(LD) - feet).max())
    entry = dict(rows=T.n, feet_floor=floor, feet_gate=gate, feet_error=err, feet_error_against_chain=err_chain)
    if quaternion:
        efloor = float(np.abs(w_64[reg, 4:7].astype(LD) - w_ld[reg, 4:7]).max())
        entry.update(euler_floor=efloor, euler_gate=lc.gate(efloor, lc.EULER_BOUND),
                     euler_error=float(np.abs(got[reg, 4:7].astype(LD) - w_ld[reg, 4:7]).max()))
        by = {n: T.n_regular + j for j, n in enumerate(T.special)}
        assert T.status[0, by["pitch+"]] & tracking.GIMBAL and T.status[0, by["pitch-"]] & tracking.GIMBAL
        assert abs(got[by["pitch+"], 5] - np.pi / 2) <= 4 * np.spacing(np.pi / 2) and abs(got[by["pitch-"], 5] + np.pi / 2) <= 4 * np.spacing(np.pi / 2)
        assert np.abs(got[by["norm3"], 4:19] - got[by["unit"], 4:19]).max() <= 8 * U + lc.FEET_BOUND
        for n in ("zero", "nan", "inf"):
            assert not np.isfinite(got[by[n], 4:19]).any() and not T.status[0, by[n]] & tracking.GIMBAL, n
    else:
        assert np.array_equal(bits(got[reg, 1:7]), bits(T.meas[reg, 0:6]))
    lc.record("k_track %s" % ("quaternion" if quaternion else "euler"), entry)
    assert err <= gate and err_chain <= gate, entry
    if quaternion:
        assert entry["euler_error"] <= entry["euler_gate"], entry


@pytest.mark.parametrize("cls", CLASSES)
def test_joint_rows_angles_come_back_through_k_track(rig, cls):
    """The round trip across the two kernels' copies of the chain: k_joint_rows' own angles of the class's probes as measured
    angles, the measured pose the plan's: the foot error columns of the unflagged legs are within 128 u m."""
    from qtos_amd import capi
    keep = [i for i, p in enumerate(rig.probes) if p.cls == cls]
    meas = np.stack([np.concatenate([rig.probes[i].com, rig.probes[i].euler, rig.tick[i, 0, 1:13]]) for i in keep])[:, None, :]
    rows, _, _, _ = rig.P.track(rig.nodes[keep], 0.0, meas, capi.track_params(hz=lc.HZ, n_rows=1, delay=0))
    entry = {}
    for j, i in enumerate(keep):
        assert rows[j, 0, 19] == 0
        legs = [e for e in range(4) if leg_bits(rig.tick_st[i, 0], e) == 0]
        entry[rig.probes[i].name] = dict(unflagged_legs=legs, worst_foot_error=max([float(rows[j, 0, 20 + e]) for e in legs], default=0.0))
    lc.record("k_joint_rows through k_track %s" % cls, dict(gate=lc.ROUND_TRIP_BOUND, probes=entry))
    for name, v in entry.items():
        assert v["worst_foot_error"] <= lc.ROUND_TRIP_BOUND, (name, v)
    assert cls in ("beyond", "inside") or any(v["unflagged_legs"] for v in entry.values())


def test_fit_and_qp_torques_on_the_angle_probes(rig):
    """k_force_fit and k_force_qp with a joint table of the angle probes on a static pose plan in equilibrium: columns 20 .. 31 are
    -J_geo(q)^T R^T f of the kernel's own forces (columns 1 .. 12) within the torque gate, and the two kernels' torques agree
    to the bit on rows the QP does not limit."""
    from qtos_amd import capi, force_qp, joints
    p = lc.fit_probe()
    table = lc.joint_table()
    n = len(table)
    joint = np.zeros((1, n, 37))
    joint[0, :, 1:13] = table
    nodes = p.nodes(rig.L)[None]
    fit, fit_st, _ = rig.P.force_fit(nodes, 0.0, capi.fit_params(lc.cfg(), hz=TRACK_HZ, n_rows=n), joint=joint)
    qp, _, qp_st, _ = rig.P.force_qp(nodes, 0.0, capi.qp_params(lc.cfg(), hz=TRACK_HZ, n_rows=n), joint=joint)
    R = joints.rotation(p.euler, LD)
    entry = {}
    for name, rows in (("k_force_fit", fit[0]), ("k_force_qp", qp[0])):
        assert np.isfinite(rows[:, 1:13]).all() and np.abs(rows[:, 1:13]).max() > 1
        err = floor = bound = 0.0
        for e in range(4):
            f = rows[:, 1 + 3 * e:4 + 3 * e]
            f_b = np.einsum("ji,nj->ni", R, f.astype(LD))
            _, Jg = jc.chain(e, table[:, 3 * e:3 * e + 3], LD)
            want = -np.einsum("nji,nj->ni", Jg, f_b)
            st64 = joints.feed_forward(e, table[:, 3 * e:3 * e + 3], np.broadcast_to(p.euler, (n, 3)), f, lc.statement_params(), F64)
            gates = np.minimum(np.maximum(8 * np.abs(st64.astype(LD) - want).max(axis=1).astype(F64), lc.TORQUE_BOUND * np.abs(f).sum(axis=1)), CAP)
            e_rows = np.abs(rows[:, 20 + 3 * e:23 + 3 * e].astype(LD) - want).max(axis=1).astype(F64)
            worst = int(np.argmax(e_rows / np.maximum(gates, 1e-300)))           # (a swing foot has no force: error and gate 0)
            if e_rows[worst] / max(gates[worst], 1e-300) >= err / max(bound, 1e-300):
                err, bound = float(e_rows[worst]), float(gates[worst])
            floor = max(floor, float(np.abs(st64.astype(LD) - want).max()))
            assert (e_rows <= gates).all(), (name, e, worst, e_rows[worst], gates[worst])
        entry[name] = dict(rows=n, worst_error=err, its_gate=bound, float64_floor=floor)
    # the two kernels: where the QP does not limit a row and its forces are the fit's to the bit (on the other free rows the two
    # kernels' forces differ in their last places: tests/test_gpu_force_qp.py holds them to 1e-6 N), so are the torques
    free = (qp_st[0] & force_qp.LIMITED) == 0
    same = free & (bits(fit[0, :, 1:13]) == bits(qp[0, :, 1:13])).all(axis=1)
    entry["rows the QP does not limit"] = dict(rows=int(free.sum()), with_the_fits_forces_to_the_bit=int(same.sum()),
                                               largest_force_difference=float(np.abs(fit[0, free, 1:13] - qp[0, free, 1:13]).max()))
    lc.record("fit_foot_out torques", entry)
    assert free.any() and same.any()
    assert np.array_equal(bits(fit[0, same, 20:32]), bits(qp[0, same, 20:32]))
