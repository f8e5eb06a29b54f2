"""The feedback hand-over on the MI355X (pytest -m gpu): k_start_feedback against the statement of its rule (qtos_amd/feedback.py).

Shapes.  B = 5 windows of the golden walk at HZ = 2 rows per second, hand-over rows ROWS = 5, 0, 7, 3, 6, so that the measured row
k = r - 1 of every window lies in a ring of capacity 7, whose cursors make (cursor + k) mod 7 wrap.  Window 1 has no measurement
(r = 0), window 2 is measured 0.08 m ahead (the clip of 0.05 m acts), window 3's base is measured 0.045 m off in x and y with its
feet where they are planned (joint angles by joints.leg_ik: not a rigid shift, so the corrected feet leave their box and the window
falls back), windows 0 and 4 are shifted rigidly.  The handle holds three constant heightfields, 0, 0.01 and 0.03 m: with map_id
NULL every z snaps to 0, with map_id = 0, 1, 2, 1, 0 to the map's constant, and 0.03 m is more than snap_tol.  Gains 0.75.

Bit-exact.  The plan-row part p is qtos_sample_csv's columns 1 .. 18 of row k and the measured pose m is qtos_track's columns 1 ..
18 of the same row, both from the device: err_out must be clip(wrap(m - p)) in float64, to the bit, and the corrected columns
start + gain * err of the kernel's own err, one rounded product and one rounded sum.  So are the snapped z, the copies of the
windows that fall back or have no measurement, the sentinels of what is not written, goal = start + goal_step on the kernel's own
start, and the status words: the test checks in longdouble that no window stands within 1e-9 of a gate's edge.

Accuracy gates against the longdouble rule (feedback.start_feedback with the measured pose in longdouble and the same p): as
tests/test_gpu_track.py, no document with ROCm's ulp figures is installed next to the compiler, so 4 ulp are ASSUMED for each of
sqrt, sin, cos, atan2 and asin, and with u = 2^-53 that file's chain gives the measured pose M = 0 for the CoM (copied), 0 for the
Euler angles in Euler mode and 256 u rad in quaternion mode, 128 u m for the feet.  Then e = m - p is one rounding, u |e|; gain *
e one more, u |gain e|; start + gain e a third, u |result|: gate = gain M + u (gain |e| + |gain e| + |result|).  The yaw's
remainder is exact.  Nothing is taken from the kernel.  The worst case in units of the gate goes through record()."""
import ctypes as C
import json
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_gv

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
HZ = 2.0
B, CAP = 5, 7
ROWS = np.array([5, 0, 7, 3, 6], np.int32)
CURSOR = np.array([3, 12, 6, 0, 5], np.int64)
T0 = np.array([3.756, 0.0, 11.25, 0.5, 2.0])
MAPS = np.array([0, 1, 2, 1, 0], np.int32)
HEIGHTS = (0.0, 0.01, 0.03)
GAIN = 0.75
GOAL_STEP = np.array([[0.3, 0.01 * b, 7.0] for b in range(B)])
M_FEET, M_EULER_QUAT = 128 * U, 256 * U
LLP = C.POINTER(C.c_longlong)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def record(name, entry):
    print("feedback accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_FEEDBACK_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def quat_of(euler):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll), float64."""
    e = np.asarray(euler, F64)
    sr, cr, sp_, cp, sy, cy = (f(e[..., i] / 2) for i in range(3) for f in (np.sin, np.cos))
    return np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], -1)


class Ctx:
    """The planner with its three heightfields, the golden nodes, the hand-over start vectors (qtos_sample_csv's row r) and the
    measured rows of the B windows, as a table [B, 7, 18]."""

    def __init__(self):
        from oracle import splines as sp
        from qtos_amd import capi, joints
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.cfg = PlannerConfig.reference_compat()
        self.P = Planner(self.cfg, max_batch=8)
        self.maps = np.stack([np.full((30, 20), h) for h in HEIGHTS])
        self.P.set_heightfields(self.maps, 0.1)
        self.L = sp.layout(self.cfg)
        self.x = np.array(load_gv("gv1")["x"])
        self.nodes = np.repeat(self.x[None], B, axis=0)
        self.sample = self.P.sample(self.nodes, T0, hz=HZ, n_rows=CAP + 1)                 # rows 0 .. 7 of every window
        self.start = np.stack([self.sample[b, ROWS[b], 1:25] for b in range(B)])
        self.start.setflags(write=False)
        joint, jst = self.P.joint_rows(self.nodes, T0, capi.joint_params(hz=HZ, n_rows=CAP, tau_max=0.0))
        meas = np.concatenate([self.sample[:, :CAP, 1:7], joint[:, :, 1:13]], 2)
        rng = np.random.default_rng(51)
        meas[0, :, 0:3] += np.array([0.010, -0.005, 0.0])
        meas[4, :, 0:3] += np.array([-0.004, 0.008, 0.0])
        meas[[0, 4]] += 1e-4 * rng.standard_normal((2, CAP, 18))
        meas[2, :, 0] += 0.08
        for k in range(CAP):                                     # window 3: the base is off, the feet are where they are planned
            com = self.sample[3, k, 1:4] + np.array([0.045, -0.045, 0.0])
            meas[3, k, 0:3] = com
            for e in range(4):
                p_b, _ = joints.base_frame(com, self.sample[3, k, 4:7], self.sample[3, k, 7 + 3 * e:10 + 3 * e], 0.015, dtype=F64)
                q, _ = joints.leg_ik(e, p_b, dtype=F64)
                meas[3, k, 6 + 3 * e:9 + 3 * e] = q
        self.meas = meas
        self.meas.setflags(write=False)

    def height(self, mode=1):
        from qtos_amd import feedback
        return feedback.terrain_lookup(self.maps, 0.1, mode=mode)

    def params(self, **kw):
        from qtos_amd import capi
        a = dict(hz=HZ, gain_pos=GAIN, gain_ang=GAIN, gain_foot=GAIN)
        a.update(kw)
        return capi.feedback_params(self.cfg, **a)

    def ring(self, meas):
        """The table's rows at (cursor + j) mod CAP of a NaN ring."""
        ring = np.full_like(meas, np.nan)
        for b in range(B):
            ring[b, (CURSOR[b] + np.arange(CAP)) % CAP] = meas[b]
        return ring

    def call(self, params, meas, cursor=None, map_id=None, goal=True, rows=ROWS, nodes=None, t0=T0, start=None):
        n = len(rows)
        return self.P.start_feedback(self.nodes if nodes is None else nodes, t0, rows, meas, params, self.start if start is None else start,
                                     cursor=cursor, map_id=map_id, goal_step=GOAL_STEP if goal else None,
                                     goal=np.full((n, 3), -7.5) if goal else None, err=np.full((n, 18), -7.5), status=np.full(n, -7, np.int32))


_ctx = []


@pytest.fixture(scope="module")
def ctx():
    if not _ctx:
        _ctx.append(Ctx())
    yield _ctx[0]


@pytest.fixture(scope="module", autouse=True)
def _close():
    yield
    for c in _ctx:
        c.P.close()
    _ctx.clear()


def wrap_clip(e, p):
    """err_out of a window from m - p, float64: the yaw's remainder and the clips; (err, clipped)."""
    e = np.array(e, F64)
    e[5] = math.remainder(float(e[5]), 2 * math.pi)
    c = np.array([p.max_pos] * 3 + [p.max_ang] * 3 + [p.max_foot] * 12)
    out = np.clip(e, -c, c)
    return out, bool((out != e).any())


def rom_margin(cfg, c):
    """How far the nearest |d_f[i]| of a start vector is from its bound max_deviation[i] + rom_tol, in longdouble."""
    from qtos_amd import joints
    c = np.asarray(c).astype(LD)
    R = joints.rotation(c[3:6], LD)
    d = np.array([R.T @ (c[6 + 3 * f:9 + 3 * f] - c[0:3]) - np.array(cfg.nominal_stance[f], LD) for f in range(4)])
    return float(np.abs(np.abs(d) - (np.array(cfg.max_deviation, LD) + LD(1e-6))).min())


def check(ctx, name, quat, ring, per_map):
    """One call of the layout against the rule: every statement of the file's docstring."""
    from qtos_amd import capi, feedback, tracking
    meas = np.array(ctx.meas)
    if quat:
        meas = np.concatenate([meas[:, :, 0:3], 1.7 * quat_of(meas[:, :, 3:6]), meas[:, :, 6:18]], 2)
    p = ctx.params(capacity=CAP if ring else 0, n_rows=0 if ring else CAP, quaternion=quat)
    fed = ctx.ring(meas) if ring else meas
    cursor = CURSOR if ring else None
    start, goal, err, status = ctx.call(p, fed, cursor=cursor, map_id=MAPS if per_map else None)
    track = ctx.P.track(ctx.nodes, T0, meas, capi.track_params(hz=HZ, n_rows=CAP, quaternion=quat))[0]
    height = ctx.height()
    worst = dict(pos=0.0, euler=0.0, feet=0.0)
    for b in range(B):
        r = int(ROWS[b])
        mid = int(MAPS[b]) if per_map else 0
        w64 = feedback.start_feedback(ctx.L, ctx.x, T0[b], r, fed[b], p, ctx.start[b], height, mid, GOAL_STEP[b], int(CURSOR[b]) if ring else 0, F64)
        if r == 0:                                                                       # no measurement: nothing but the status is written
            assert status[b] == w64[3] == feedback.NO_MEASUREMENT
            assert np.array_equal(bits(start[b]), bits(ctx.start[b])) and (err[b] == -7.5).all() and (goal[b] == -7.5).all()
            continue
        k = r - 1
        e_want, clipped = wrap_clip(track[b, k, 1:19] - ctx.sample[b, k, 1:19], p)      # m and p are the device's own: to the bit
        assert np.array_equal(bits(err[b]), bits(e_want)), (name, b)
        assert status[b] == w64[3], (name, b, status[b], w64[3])
        assert bool(status[b] & feedback.CLIPPED) == clipped == (b == 2)
        assert bool(status[b] & feedback.FALLBACK) == (b == 3) and bool(status[b] & feedback.CORRECTED) == (b != 3)
        assert np.array_equal(bits(goal[b, 0:2]), bits(start[b, 0:2] + GOAL_STEP[b, 0:2])) and goal[b, 2] == -7.5
        assert np.array_equal(bits(start[b, 18:24]), bits(ctx.start[b, 18:24]))          # the velocities stay the plan's
        if b == 3:                                                                       # fallback: the input, to the bit
            assert np.array_equal(bits(start[b]), bits(ctx.start[b]))
            continue
        want = ctx.start[b, 0:18] + GAIN * err[b]                                        # one rounded product, one rounded sum
        z = np.zeros(18, bool)
        z[8:18:3] = True
        assert np.array_equal(bits(start[b, 0:18][~z]), bits(want[~z])), (name, b)
        assert (start[b, 0:18][z] == HEIGHTS[mid]).all()
        # against the longdouble rule on the same p: m in longdouble
        m_ld = tracking.measured_pose(fed[b, (CURSOR[b] + k) % CAP if ring else k], p, LD)
        e_ld = m_ld - ctx.sample[b, k, 1:19].astype(LD)
        e_ld[5] = feedback.wrap_yaw(e_ld[5], LD)
        clip = np.array([p.max_pos] * 3 + [p.max_ang] * 3 + [p.max_foot] * 12).astype(LD)
        e_ld = np.minimum(np.maximum(e_ld, -clip), clip)
        c_ld = ctx.start[b, 0:18].astype(LD) + LD(GAIN) * e_ld
        M = np.array([0.0] * 3 + [M_EULER_QUAT if quat else 0.0] * 3 + [M_FEET] * 12)
        gate = GAIN * M + U * (GAIN * np.abs(err[b]) + np.abs(GAIN * err[b]) + np.abs(want))
        rel = np.abs(start[b, 0:18].astype(LD) - c_ld)[~z] / gate[~z]
        for key, sl in (("pos", slice(0, 3)), ("euler", slice(3, 6)), ("feet", slice(6, 14))):
            worst[key] = max(worst[key], float(rel[sl].max()))
        # the gates of the status word are not near: the range-of-motion margins and the clips, in longdouble
        w_ld = feedback.start_feedback(ctx.L, ctx.x, T0[b], r, fed[b], p, ctx.start[b], height, mid, None, int(CURSOR[b]) if ring else 0, LD)
        assert w_ld[3] == status[b]
        if b != 2:
            assert float(np.abs(np.abs(w_ld[2]) - clip).min()) > 1e-9
        assert float(np.abs(np.abs(LD(HEIGHTS[mid]) - c_ld[z]) - LD(p.snap_tol)).min()) > 1e-9
        assert rom_margin(ctx.cfg, w_ld[0]) > 1e-9
    record(name, dict(worst_in_units_of_the_gate=worst))
    assert max(worst.values()) <= 1.0, (name, worst)
    return start, goal, err, status


@pytest.mark.parametrize("per_map", [False, True])
@pytest.mark.parametrize("ring", [False, True])
@pytest.mark.parametrize("quat", [False, True])
def test_layout_and_numbers(ctx, quat, ring, per_map):
    check(ctx, "%s %s %s" % ("quaternion" if quat else "euler", "ring" if ring else "table", "maps" if per_map else "map 0"), quat, ring, per_map)


def test_fallback_margin_ring_is_the_table_and_options(ctx):
    """The fallback of window 3 is not near the gate; ring and table give the same bits; latency, the snap switched off, the zero
    filter and gains of 0."""
    from qtos_amd import feedback, joints
    p = ctx.params(n_rows=CAP)
    table = ctx.call(p, ctx.meas)
    ring = ctx.call(ctx.params(capacity=CAP), ctx.ring(np.array(ctx.meas)), cursor=CURSOR)
    for a, b in zip(table, ring):
        assert np.array_equal(bits(a), bits(b)) if a.dtype == F64 else np.array_equal(a, b)
    # window 3 in longdouble: the largest excess over the box is millimetres, not roundings
    k = int(ROWS[3]) - 1
    c = ctx.start[3, 0:18].astype(LD) + LD(GAIN) * table[2][3].astype(LD)
    c[8:18:3] = 0
    R = joints.rotation(c[3:6], LD)
    d = np.array([R.T @ (c[6 + 3 * f:9 + 3 * f] - c[0:3]) - np.array(ctx.cfg.nominal_stance[f], LD) for f in range(4)])
    excess = float((np.abs(d) - np.array(ctx.cfg.max_deviation, LD)).max())
    assert excess > 1e-3 and table[3][3] & feedback.FALLBACK
    # latency of one second: two rows earlier, clamped at row 0
    lat = ctx.params(n_rows=CAP, latency=1.0)
    got = ctx.call(lat, ctx.meas)
    for b in (0, 2, 4):
        k = max(int(ROWS[b]) - 2, 0)
        w = feedback.start_feedback(ctx.L, ctx.x, T0[b], int(ROWS[b]), ctx.meas[b], lat, ctx.start[b], ctx.height(), 0, None, 0, F64)
        assert feedback.measured_row(int(ROWS[b]), lat) == (k, k) and got[3][b] == w[3]
        assert float(np.abs(got[2][b] - w[2]).max()) < 1e-12 and not np.array_equal(got[2][b], table[2][b])
    # without the snap the z columns are start + gain * err as well; with gains 0 nothing is written but err, goal and status
    off = ctx.call(ctx.params(n_rows=CAP, snap=False), ctx.meas, map_id=MAPS)
    for b in (0, 4):
        assert np.array_equal(bits(off[0][b, 0:18]), bits(ctx.start[b, 0:18] + GAIN * off[2][b])) and off[3][b] == feedback.CORRECTED
    zero = ctx.call(ctx.params(n_rows=CAP, gain_pos=0, gain_ang=0, gain_foot=0), ctx.meas, map_id=MAPS)
    assert np.array_equal(bits(zero[0]), bits(ctx.start)) and zero[3].tolist() == [0, 32, 2, 0, 0]
    assert np.array_equal(bits(zero[2][[0, 2, 3, 4]]), bits(table[2][[0, 2, 3, 4]]))
    assert np.array_equal(bits(zero[1][[0, 2, 3, 4], 0:2]), bits(ctx.start[[0, 2, 3, 4], 0:2] + GOAL_STEP[[0, 2, 3, 4], 0:2]))
    # zero filter: on the 24 numbers of the windows that did not fall back
    s2 = np.array(ctx.start)
    s2[:, 19], s2[:, 20] = 5e-5, 2e-4
    plain = ctx.call(p, ctx.meas, start=s2)
    filt = ctx.call(ctx.params(n_rows=CAP, zero_filter=True), ctx.meas, start=s2)
    for b in range(B):
        if b in (1, 3):
            assert np.array_equal(bits(filt[0][b]), bits(s2[b]))
        else:
            want = np.where(np.abs(plain[0][b]) < 1e-4, 0.0, plain[0][b])
            assert np.array_equal(bits(filt[0][b]), bits(want)) and filt[0][b, 19] == 0 and filt[0][b, 20] == 2e-4
    # without goal_step no goal is asked for
    none = ctx.call(p, ctx.meas, goal=False)
    assert none[1] is None and np.array_equal(bits(none[0]), bits(table[0]))


def test_65_windows_are_two_workgroups(ctx):
    n = 65
    idx = np.arange(n) % B
    idx[64] = 0                                                                          # (the one lane of the second workgroup has window 0's inputs)
    p = ctx.params(n_rows=CAP)
    one = ctx.call(p, ctx.meas, map_id=MAPS)
    # (the host form goes through buffers of its own: more windows than the handle's max_batch)
    many = ctx.P.start_feedback(ctx.nodes[idx], T0[idx], ROWS[idx], np.array(ctx.meas)[idx], p, np.array(ctx.start)[idx], map_id=MAPS[idx],
                                goal_step=GOAL_STEP[idx], goal=np.full((n, 3), -7.5), err=np.full((n, 18), -7.5), status=np.full(n, -7, np.int32))
    for a, b in zip(one, many):
        assert np.array_equal(bits(a[idx]), bits(b)) if a.dtype == F64 else np.array_equal(a[idx], b)
    assert np.array_equal(bits(many[0][64]), bits(many[0][0])) and many[3][64] == many[3][0] == one[3][0]


def test_device_form_next_to_an_open_plan_call(ctx):
    """Queued on a side stream while a plan call is open: its results are the host form's, and the plan's outputs are the bits of
    a run without it."""
    import torch
    from qtos_amd import workloads
    P = ctx.P
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    p = ctx.params(n_rows=CAP)
    host = ctx.call(p, ctx.meas, map_id=MAPS)
    s0, g0 = workloads.flat_goals(4, seed=3)
    main, side = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    runs = []
    for with_feedback in (False, True):
        d_s, d_g = torch.as_tensor(s0, **f64), torch.as_tensor(g0, **f64)
        nodes, viol = torch.zeros((4, P.n), **f64), torch.zeros(4, **f64)
        status, iters = torch.full((4,), -1, **i32), torch.zeros(4, **i32)
        fb = dict(nodes=torch.as_tensor(ctx.nodes, **f64), t0=torch.as_tensor(T0, **f64), row=torch.as_tensor(ROWS, **i32),
                  meas=torch.as_tensor(np.array(ctx.meas), **f64), map=torch.as_tensor(MAPS, **i32), start=torch.as_tensor(np.array(ctx.start), **f64),
                  gs=torch.as_tensor(GOAL_STEP, **f64), goal=torch.full((B, 3), -7.5, **f64), err=torch.full((B, 18), -7.5, **f64),
                  st=torch.full((B,), -7, **i32))
        torch.cuda.synchronize()
        rc = P.lib.qtos_plan_submit(P.h, 4, d_s.data_ptr(), d_g.data_ptr(), None, None, nodes.data_ptr(), status.data_ptr(), iters.data_ptr(),
                                    viol.data_ptr(), C.c_void_p(main.cuda_stream))
        assert rc == 0, P.lib.qtos_last_error(P.h)
        if with_feedback:                                                                  # (the plan call is open: no wait, no poll yet)
            rc = P.lib.qtos_start_feedback_device(P.h, B, C.byref(p), fb["nodes"].data_ptr(), fb["t0"].data_ptr(), fb["row"].data_ptr(), None,
                                                  fb["meas"].data_ptr(), fb["map"].data_ptr(), fb["start"].data_ptr(), fb["gs"].data_ptr(),
                                                  fb["goal"].data_ptr(), fb["err"].data_ptr(), fb["st"].data_ptr(), C.c_void_p(side.cuda_stream))
            assert rc == 0, P.lib.qtos_last_error(P.h)
        P.wait()
        assert P.poll()
        torch.cuda.synchronize()
        runs.append((nodes.cpu().numpy(), status.cpu().numpy(), iters.cpu().numpy(), viol.cpu().numpy()))
        if with_feedback:
            got = (fb["start"].cpu().numpy(), fb["goal"].cpu().numpy(), fb["err"].cpu().numpy(), fb["st"].cpu().numpy())
            for a, b in zip(host, got):
                assert np.array_equal(bits(a), bits(b)) if a.dtype == F64 else np.array_equal(a, b)
    assert (runs[0][1] == 0).all()
    for a, b in zip(*runs):
        assert np.array_equal(bits(a), bits(b)) if a.dtype == F64 else np.array_equal(a, b)


def test_argument_checks(ctx):
    from qtos_amd import capi
    p = ctx.params(capacity=CAP)
    meas, start, gs = ctx.ring(np.array(ctx.meas))[:1], np.array(ctx.start[:1]), np.array(GOAL_STEP[:1])

    def call(**kw):
        a = dict(h=ctx.P.h, b=1, s=p, nodes=ctx.nodes[:1], t0=T0[:1], row=ROWS[:1], cur=CURSOR[:1].copy(), meas=meas, start=start.copy(),
                 gs=gs, goal=np.zeros((1, 3)), err=np.zeros((1, 18)), st=np.zeros(1, np.int32))
        a.update(kw)
        return ctx.P.lib.qtos_start_feedback(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]),
                                             capi._ip(a["row"]), None if a["cur"] is None else a["cur"].ctypes.data_as(LLP), capi._dp(a["meas"]),
                                             None, capi._dp(a["start"]), capi._dp(a["gs"]), capi._dp(a["goal"]), capi._dp(a["err"]),
                                             capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            setattr(s, key, v)
        return s
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null t0": call(t0=None), "null row": call(row=None), "null meas": call(meas=None), "null start": call(start=None),
           "null status": call(st=None), "ring without cursor": call(cur=None), "capacity < 0": call(s=params(capacity=-1)),
           "table without rows": call(s=params(capacity=0, n_rows=0)), "first_row -1": call(s=params(first_row=-1)),
           "first_row 1000001": call(s=params(first_row=1000001)), "latency < 0": call(s=params(latency=-0.001)),
           "gain_pos < 0": call(s=params(gain_pos=-0.1)), "gain_ang > 1": call(s=params(gain_ang=1.5)), "gain_foot nan": call(s=params(gain_foot=float("nan"))),
           "max_pos 0": call(s=params(max_pos=0.0)), "max_ang < 0": call(s=params(max_ang=-1.0)), "max_foot 0": call(s=params(max_foot=0.0)),
           "l_upper 0": call(s=params(l_upper=0.0)), "l_lower 0": call(s=params(l_lower=0.0)),
           "goal_step without goal": call(goal=None), "goal without goal_step": call(gs=None)}
    assert all(v == -1 for v in got.values()), got
    assert call() == 0 and call(s=params(first_row=1000000)) == 0 and call(gs=None, goal=None) == 0 and call(err=None) == 0
    assert call(s=params(gain_pos=0.0, gain_ang=1.0)) == 0
    dev = ctx.P.lib.qtos_start_feedback_device(None, 1, C.byref(p), None, None, None, None, None, None, None, None, None, None, None, None)
    assert dev == -1


def test_feedback_from_plain_c(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "feedback_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "feedback_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.reference_compat())))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_feedback=%d feedback_null=-1 feedback_device_null=-1" % C.sizeof(capi.QtosFeedback)
    assert lines[1] == "bad_args=" + ",".join(["-1"] * 8)
    assert lines[2] == "plan rc=0 status=0,0"
    kv = dict(t.split("=") for t in lines[3].replace("feedback rc", "feedback_rc").split())
    assert int(kv["feedback_rc"]) == 0 and kv["status"] == "1,1" and int(kv["mismatches"]) == 0
    assert float(kv["largest_miss"]) < 1e-12                          # start - (hand-over + drift), x and y of CoM and feet
    assert lines[4] == "replan rc=0 status=0,0"


def test_shifted_windows_replan_from_the_measured_state():
    """B = 4, three replans of 420 rows, the robot measured where it is planned, shifted rigidly by D: after every replan start[:, 0:2] is the
    hand-over's + gain * D, feedback_status is 1 and every plan converges; with gains of 0 the plans of all three replans are the
    bits of a set without `feedback`."""
    import torch
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    nb, cap, seg, gain = 4, 1300, 420, 0.5      # (row 420: the walk's hind left foot is down again at 0.37 s, the front left lifts at 0.49 s)
    D = np.array([0.010, -0.005, 0.0])
    start, goal = workloads.flat_goals(nb, seed=7)
    cfg = PlannerConfig.reference_compat()
    P = Planner(cfg, max_batch=nb)
    host = lambda t: t.cpu().numpy().copy()
    log = []

    def fill(W):          # on the windows' stream, behind the hand-over and the joint rows: measured = planned + D, the commanded angles
        assert torch.cuda.current_stream(W.dev) == W.stream
        rows = torch.empty((nb, seg, 37), dtype=torch.float64, device=W.dev)
        rc = P.lib.qtos_sample_csv_device(P.h, nb, W.nodes.data_ptr(), W.t0.data_ptr(), C.c_double(1000.0), seg, rows.data_ptr(),
                                          C.c_void_p(W.stream.cuda_stream))
        assert rc == 0
        c = seg * len(log)
        if c + seg <= cap:
            W.meas_traj[:, c:c + seg, 0:6] = rows[:, :, 1:7]
            W.meas_traj[:, c:c + seg, 0:3] += torch.as_tensor(D, dtype=torch.float64, device=W.dev)
            W.meas_traj[:, c:c + seg, 6:18] = W.joint_traj[:, c:c + seg, 1:13]
        log.append(dict(handed=W.start.clone(), planned=rows[:, seg - 1, 1:3].clone()))
    try:
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, feedback={})
        runs = {}
        for name, fb in (("none", None), ("zero", dict(gain_pos=0, gain_ang=0, gain_foot=0, snap=False)),
                         ("half", dict(gain_pos=gain, gain_ang=gain, gain_foot=gain))):
            del log[:]
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(tau_max=3.0),
                               track=dict(delay=3, fill=fill), feedback=fb, stream=torch.cuda.Stream())
            if fb is None:
                assert W._feedback is None and not hasattr(W, "feedback_status") and not hasattr(W, "feedback_err")

                def never(*a):
                    raise AssertionError("a feedback call was queued")
                W._start_feedback = never
            W.replan()
            torch.cuda.synchronize()
            plans = []
            for i in range(3):
                W.replan()
                torch.cuda.synchronize()
                assert (host(W.row) == seg).all() and (host(W.status) == 0).all(), (name, i, host(W.status))
                plans.append(host(W.nodes))
                if name == "half":
                    st, handed, planned = host(W.start), host(log[i]["handed"]), host(log[i]["planned"])
                    assert (host(W.feedback_status) == 1).all(), host(W.feedback_status)
                    # fill rounds planned + D (u |p + D|), the kernel m - p (u |e|), gain * e (u |gain e|) and the sum (u |result|)
                    gate = U * (2 * np.abs(planned + D[0:2]) + 2 * np.abs(gain * D[0:2]) + np.abs(st[:, 0:2]))
                    miss = np.abs(st[:, 0:2].astype(LD) - (handed[:, 0:2].astype(LD) + LD(gain) * D[0:2].astype(LD)))
                    record("shifted windows replan %d" % i, dict(worst_in_units_of_the_gate=float((miss / gate).max())))
                    assert (miss <= gate).all(), (i, miss, gate)
                    assert np.array_equal(bits(host(W.goal)[:, 0:2]), bits(st[:, 0:2] + host(W.goal_step)[:, 0:2]))
                    assert np.abs(host(W.feedback_err)[:, 0:2] - D[0:2]).max() < 1e-12
            runs[name] = plans
        for a, b in zip(runs["none"], runs["zero"]):
            assert np.array_equal(bits(a), bits(b))
        assert not np.array_equal(bits(runs["none"][0]), bits(runs["half"][0]))
    finally:
        P.close()
