"""The joint-rows kernel on the MI355X (pytest -m gpu): k_joint_rows against the longdouble statement of the rule (qtos_amd/joints.py)
and against the URDF's chain (tests/joint_chain.py) on three plans, its motor law against numpy to the bit, the 1 kHz tick, the
joint ring of ShiftedWindows against table-mode rows, a non-default stream, the host form and the calls from plain C.

Accuracy gates.  The angles and the forward-kinematics round trip are held to the larger of 8 x the float64 numpy floor measured
here and a bound propagated from the device math library's errors; no document with ROCm's ulp figures is installed next to the
compiler, so 4 ulp are ASSUMED for each of sqrt, sin, cos, atan2 and acos.  With u = 2^-53 (one ulp of v is at most 2 u |v|):

  p_b      six sines / cosines at 8 u each, products and sums of R^T (foot - com) with |foot - com| <= 0.5 m: 10 u m
  c3       r dr / l^2 with r <= 0.32 m, l^2 = 0.0256 m^2: 125 u, and 12 u of its own sums: 140 u; q3 = acos(c3) turns that into
           140 u / |sin q3| and adds 4 ulp of a result below pi: 25 u
  q1, q2   two atan2 (4 ulp of at most pi / 2 each: 13 u), the sine and cosine of q3 (8 u), the inputs' 10 u m over levers of
           0.2 m and more (50 u), sqrt's 8 u, and half of q3's error
  angles   (128 + 140 / |sin q3|) u per joint and row
  FK       the error of q3 along the singular direction cancels in q2 (q2 is formed with the sine and cosine of the rounded
           q3), so the foot is off by p_b's 10 u m and the angles' well-conditioned part over the leg's length 0.32 m: 64 u m
Every gate is capped at 1e-12.  qdot and tau_ff are held, by the residuals of tests/test_joints_cpu.py, to 8 x the float64
statement's own distance from its longdouble form, capped at 1e-12.  Measured on an MI355X (profiles/joint_accuracy.json), the
worst of the three plans: angles 3.4e-14 rad off the longdouble statement at a float64 numpy floor of 5.9e-14 rad (0.12 of the
gate at the worst row), FK round trip 1.5e-15 m (floor 1.8e-15 m), |J_geo qdot - v_b| 4.3e-14 (floor 3.8e-13), tau_ff 4.4e-14 N m
(floor 4.3e-14 N m)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import joint_chain as jc
from conftest import ROOT, load_gv

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
HZ, N_ROWS = 200.0, 1100             # three 512-row tiles, the last one partial; rows 1001 .. 1099 lie past the horizon
CAP = 1e-12
MARGIN = 1e-12                       # status is compared where the longdouble c3 and h^2 are further than this from their thresholds


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def record(name, entry):
    print("joint accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_JOINT_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


class Case:
    """One plan: its planner, nodes, the kernel's table (no measured state, no clip: columns 25 .. 36 are tau_ff) and the
    statement's rows in longdouble and float64."""

    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, joints, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name = name
        cfg = PlannerConfig.reference_compat(gait="trot") if name == "trot" else PlannerConfig.reference_compat()
        self.P = Planner(cfg, max_batch=8)
        if name == "walk":
            self.nodes = np.array(load_gv("gv1")["x"])[None]
        elif name == "trot":
            start, goal = workloads.flat_goals(1, seed=11)
            self.nodes, status, _, _ = self.P.plan(start, goal)
            assert status[0] == 0
        else:                                                   # a step onto the ledges of exp_5: the base pitches
            hxy, cell = workloads.exp5_terrain()
            self.P.set_heightfields(hxy, cell)
            start, goal = workloads.step_goals(1, seed=1, terrain=(hxy, cell))
            self.nodes, status, _, _ = self.P.plan(start, goal)
        self.t0 = np.array([3.756])
        self.L = sp.layout(cfg)
        self.params = capi.joint_params(hz=HZ, n_rows=N_ROWS, tau_max=0.0)
        self.rows, self.status = self.P.joint_rows(self.nodes, self.t0, self.params)
        self.rows.setflags(write=False)
        self.want = {dt: joints.joint_rows(self.L, self.nodes[0], self.t0[0], HZ, 0, N_ROWS, self.params, dtype=dt) for dt in (LD, F64)}
        # the statement's Cartesian rows, feet in the base frame and margins, in longdouble
        t = np.minimum(np.arange(N_ROWS) / HZ, self.L.T)
        self.cart = sp.sample_rows(self.L, self.nodes[0], self.t0[0], HZ, N_ROWS, LD)
        fv = [sp.eval_spline(self.L, 2 + e, self.nodes[0], t, 1, LD) for e in range(4)]
        self.p_b, self.v_b, self.decided = [], [], []
        for e in range(4):
            p, v = joints.base_frame(self.cart[:, 1:4], self.cart[:, 4:7], self.cart[:, 7 + 3 * e:10 + 3 * e], 0.015, self.cart[:, 19:22],
                                     self.cart[:, 22:25], fv[e], LD)
            c3, h2 = joints.ik_margins(e, p, dtype=LD)
            self.p_b.append(p)
            self.v_b.append(v)
            self.decided.append((np.abs(c3 - 1) > MARGIN) & (np.abs(c3 + 1) > MARGIN) & (np.abs(h2) > MARGIN))

    def leg_ok(self, e):
        """Rows where leg e has no status bit in the statement."""
        return ((self.want[LD][1] >> e) & 0x111) == 0


_cases = {}


@pytest.fixture(params=["walk", "trot", "exp5"])
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_planners():
    yield
    for c in _cases.values():
        c.P.close()
    _cases.clear()


def test_time_stamps_and_status(case):
    table = case.P.sample(case.nodes, case.t0, hz=HZ, n_rows=N_ROWS)
    assert case.rows.shape == (1, N_ROWS, 37) and case.status.shape == (1, N_ROWS) and case.status.dtype == np.int32
    assert np.array_equal(bits(case.rows[0, :, 0]), bits(table[0, :, 0]))            # qtos_sample_csv's time stamps, to the bit
    assert N_ROWS > 2 * 512 and (N_ROWS - 1) / HZ > case.L.T                           # a partial third tile, rows past the horizon
    tail = case.rows[0, int(case.L.T * HZ) + 1:, 1:]
    assert np.array_equal(bits(tail), bits(np.broadcast_to(tail[0], tail.shape)))     # behind the horizon the plan's last state
    want = case.want[LD][1]
    mask = np.zeros(N_ROWS, np.int32)
    for e in range(4):
        mask |= np.where(case.decided[e], 0x111 << e, 0).astype(np.int32)
    print("[%s] flagged rows: %d of %d, undecided legs: %d" % (case.name, int((want != 0).sum()), N_ROWS,
                                                                int(sum((~d).sum() for d in case.decided))))
    assert ((case.status[0] & mask) == (want & mask)).all()
    assert (case.status[0] & ~0xfff) .max() == 0
    if case.name == "exp5":
        assert np.abs(case.cart[:, 5]).max() > 1e-3                                    # the base does pitch


def test_angles_and_fk_round_trip(case):
    q_gpu, (w_ld, _), (w_64, _) = case.rows[0, :, 1:13], case.want[LD], case.want[F64]
    entry = {}
    for e in range(4):
        sl, ok = slice(3 * e, 3 * e + 3), case.leg_ok(e) & (((case.status[0] >> e) & 0x111) == 0)
        q_ld = w_ld[:, 1 + 3 * e:4 + 3 * e]
        s3 = np.abs(np.sin(q_ld[:, 2])).astype(F64)
        bound = U * (128 + 140 / np.maximum(s3, 1e-300))
        floor_q = float(np.abs(w_64[:, 1 + 3 * e:4 + 3 * e] - q_ld)[ok].max())
        gate_q = np.minimum(np.maximum(8 * floor_q, bound), CAP)
        err_q = np.abs(q_gpu[:, sl] - q_ld).astype(F64).max(axis=1)
        foot_gpu, _ = jc.chain(e, q_gpu[:, sl], LD)
        foot_64, _ = jc.chain(e, w_64[:, 1 + 3 * e:4 + 3 * e], LD)
        floor_fk = float(np.abs(foot_64 - case.p_b[e])[ok].max())
        gate_fk = min(max(8 * floor_fk, 64 * U), CAP)
        err_fk = float(np.abs(foot_gpu - case.p_b[e])[ok].max())
        entry["leg%d" % e] = dict(q_floor=floor_q, q_error=float(err_q[ok].max()), q_worst_over_gate=float((err_q / gate_q)[ok].max()),
                                  fk_floor=floor_fk, fk_gate=gate_fk, fk_error=err_fk)
        # a straight leg of the statement is a straight leg of the kernel
        both = ~case.leg_ok(e) & (((case.status[0] >> e) & 1) == 1)
        assert (q_gpu[both, 3 * e + 2] == 0).all()
    record("angles %s" % case.name, entry)
    for e in range(4):
        v = entry["leg%d" % e]
        assert v["q_worst_over_gate"] <= 1.0, (case.name, e, v)
        assert v["fk_error"] <= v["fk_gate"], (case.name, e, v)


def test_rates_and_feed_forward(case):
    from qtos_amd import joints
    g = case.rows[0]
    (w_ld, _), (w_64, _) = case.want[LD], case.want[F64]
    R = joints.rotation(case.cart[:, 4:7], LD)
    res, floor = dict(qdot=0.0, tau_ff=0.0), dict(qdot=0.0, tau_ff=0.0)
    for e in range(4):
        sl, ok = slice(3 * e, 3 * e + 3), case.leg_ok(e) & (((case.status[0] >> e) & 0x111) == 0)
        f_b = np.einsum("nji,nj->ni", R, case.cart[:, 25 + 3 * e:28 + 3 * e])
        _, Jg = jc.chain(e, g[:, 1 + 3 * e:4 + 3 * e], LD)                 # the chain at the kernel's own angles
        _, Jl = jc.chain(e, w_ld[:, 1 + 3 * e:4 + 3 * e], LD)
        res["qdot"] = max(res["qdot"], float(np.abs(np.einsum("nij,nj->ni", Jg, g[:, 13 + 3 * e:16 + 3 * e].astype(LD)) - case.v_b[e])[ok].max()))
        res["tau_ff"] = max(res["tau_ff"], float(np.abs(g[:, 25 + 3 * e:28 + 3 * e].astype(LD) + np.einsum("nji,nj->ni", Jg, f_b)).max()))
        floor["qdot"] = max(floor["qdot"], float(np.abs(np.einsum("nij,nj->ni", Jl, w_64[:, 13 + 3 * e:16 + 3 * e].astype(LD)
                                                                     - w_ld[:, 13 + 3 * e:16 + 3 * e]))[ok].max()))
        floor["tau_ff"] = max(floor["tau_ff"], float(np.abs(w_64[:, 25 + 3 * e:28 + 3 * e].astype(LD) - w_ld[:, 25 + 3 * e:28 + 3 * e]).max()))
        flagged = ((case.status[0] >> e) & 0x111) != 0
        assert (g[flagged, 13 + 3 * e:16 + 3 * e] == 0).all()               # a leg with a status bit stands still
    gates = {k: min(8 * v, CAP) for k, v in floor.items()}
    record("rates %s" % case.name, dict(floor=floor, gate=gates, gpu_error=res))
    for k in res:
        assert res[k] <= gates[k], (case.name, k, res[k], gates[k])


def test_motor_law_is_numpys_to_the_bit(case):
    """Given the kernel's own q, qdot and tau_ff (the table without measured state and clip), every other setting of the motor
    law is joints.motor_torque in float64, bit for bit: scaled gains, both limits, with and without feed-forward."""
    from qtos_amd import capi, joints
    rng = np.random.default_rng(5)
    B = 3
    nodes, t0 = np.repeat(case.nodes, B, axis=0), np.repeat(case.t0, B)
    q, qd, tff = case.rows[0, :, 1:13], case.rows[0, :, 13:25], case.rows[0, :, 25:37]
    q_mes = q[::500][:B] + rng.uniform(-0.3, 0.3, (B, 12))
    qd_mes = rng.uniform(-3.0, 3.0, (B, 12))
    seen = set()
    for scales, tau_max, ff in (((1.0, 1.0, 1.0), 8.0, True), ((2.0, 1.5, 0.5), 3.0, True), ((2.0, 1.5, 0.5), 3.0, False),
                                ((1.0, 1.0, 1.0), 0.0, True)):
        p = capi.joint_params(hz=HZ, n_rows=N_ROWS, hip_scale=scales[0], knee_scale=scales[1], ankle_scale=scales[2], tau_max=tau_max,
                              feed_forward=ff)
        kp, kd = joints.motor_gains(20.0, 0.08, *scales)
        got, st = case.P.joint_rows(nodes, t0, p, q_mes=q_mes, qd_mes=qd_mes)
        free, _ = case.P.joint_rows(nodes, t0, p)                           # without measured values: the PD terms are left out
        for b in range(B):
            assert np.array_equal(bits(got[b, :, :25]), bits(case.rows[0, :, :25])) and np.array_equal(st[b], case.status[0])
            want = joints.motor_torque(q, qd, tff if ff else None, kp, kd, tau_max, q_mes[b], qd_mes[b])
            assert np.array_equal(bits(got[b, :, 25:37] + 0.0), bits(want + 0.0)), (scales, tau_max, ff, b)
            want = joints.motor_torque(q, qd, tff if ff else None, kp, kd, tau_max)
            assert np.array_equal(bits(free[b, :, 25:37] + 0.0), bits(want + 0.0))
            if tau_max > 0:
                seen |= {s for s, m in (("hi", got[b, :, 25:37] == tau_max), ("lo", got[b, :, 25:37] == -tau_max),
                                        ("in", np.abs(got[b, :, 25:37]) < tau_max)) if m.any()}
    assert seen == {"hi", "lo", "in"}


def test_tick_of_five_robots(case):
    """B = 5, one row each at a row index of its own, with the measured state: the table's row and joints.motor_torque,
    including torques that clip."""
    from qtos_amd import capi, joints
    B = 5
    first = np.array([0, 1, 511, 512, 1099], np.int32)
    nodes, t0 = np.repeat(case.nodes, B, axis=0), np.repeat(case.t0, B)
    p = capi.joint_params(hz=HZ, n_rows=1)                                   # kp 20, kd 0.08, t_max 8
    q, qd, tff = (case.rows[0, first, a:b] for a, b in ((1, 13), (13, 25), (25, 37)))
    q_mes, qd_mes = q.copy(), qd.copy()
    q_mes[1:] += np.linspace(-0.6, 0.6, 12)                                  # robot 0 measures the command: tau = clip(tau_ff)
    qd_mes[2:] -= 1.5
    got, st = case.P.joint_rows(nodes, t0, p, first_row=first, q_mes=q_mes, qd_mes=qd_mes)
    assert got.shape == (B, 1, 37) and st.shape == (B, 1)
    assert np.array_equal(bits(got[:, 0, :25]), bits(case.rows[0, first, :25])) and np.array_equal(st[:, 0], case.status[0, first])
    want = joints.motor_torque(q, qd, tff, np.full(12, 20.0), np.full(12, 0.08), 8.0, q_mes, qd_mes)
    assert np.array_equal(bits(got[:, 0, 25:37] + 0.0), bits(want + 0.0))
    assert np.array_equal(bits(got[0, 0, 25:37] + 0.0), bits(np.clip(tff[0], -8, 8) + 0.0))
    assert (np.abs(got[:, 0, 25:37]) == 8.0).any() and (np.abs(got[:, 0, 25:37]) < 8.0).any()
    # a full wave of the one-wave kernel, and one row more (the 512-lane kernel): the table's rows, to the bit
    for n in (64, 65):
        part, pst = case.P.joint_rows(case.nodes, case.t0, capi.joint_params(hz=HZ, first_row=100, n_rows=n, tau_max=0.0))
        assert np.array_equal(bits(part[0]), bits(case.rows[0, 100:100 + n])) and np.array_equal(pst[0], case.status[0, 100:100 + n])


def test_device_form_on_a_held_up_stream_and_partial_counts(case):
    """The device form on a non-default stream, behind other work and reading nodes made on that stream: the default stream's
    result.  Per-window counts and first rows: rows behind a window's count are not touched."""
    import torch
    from qtos_amd import capi
    dev = torch.device("cuda", 0)
    B, n = 4, 600
    counts, first = np.array([0, 1, 513, 900], np.int32), np.array([0, 7, 100, 500], np.int32)
    p = capi.joint_params(hz=HZ, n_rows=n, tau_max=0.0)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0 = torch.as_tensor(np.repeat(case.t0, B), **f64)
    d_n, d_first = torch.as_tensor(counts, device=dev), torch.as_tensor(first, device=dev)
    src = torch.as_tensor(np.repeat(case.nodes, B, axis=0), **f64)
    outs = []
    side = torch.cuda.Stream(dev)
    busy = torch.ones((2048, 2048), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        out, st = torch.full((B, n, 37), -7.5, **f64), torch.full((B, n), -7, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if stream is side:
                for _ in range(20):
                    busy = (busy @ busy).clamp_(0.0, 1.0)
            d_nodes = src + 0.0
            rc = case.P.lib.qtos_joint_rows_device(case.P.h, B, C.byref(p), d_nodes.data_ptr(), d_t0.data_ptr(), d_first.data_ptr(),
                                                   d_n.data_ptr(), None, None, None, out.data_ptr(), st.data_ptr(),
                                                   C.c_void_p(stream.cuda_stream))
            assert rc == 0, case.P.lib.qtos_last_error(case.P.h)
        stream.synchronize()
        outs.append((out.cpu().numpy(), st.cpu().numpy()))
    torch.cuda.synchronize()
    (a, sa), (b, sb) = outs
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(sa, sb)
    for w in range(B):
        m = min(int(counts[w]), n)
        k = np.minimum(first[w] + np.arange(m), N_ROWS - 1)
        assert np.array_equal(bits(a[w, :m, 1:]), bits(case.rows[0, k, 1:])) and np.array_equal(sa[w, :m], case.status[0, k])
        assert (a[w, m:] == -7.5).all() and (sa[w, m:] == -7).all()


def test_ring_of_shifted_windows_is_the_table_row_for_row():
    """Capacity 700, three segments of 300 rows: every joint ring row is the table-mode row of the same plan and index, to the bit;
    the CSV ring, the cursor and the clock are what they are without `joints`; finish() fills the joint ring with the CSV ring."""
    import torch
    from qtos_amd import capi, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    from qtos_amd.stitcher import ring_rows
    B, cap, seg = 4, 700, 300
    start, goal = workloads.flat_goals(B, seed=7)
    P = Planner(PlannerConfig.knots100(gait="trot"), max_batch=B)
    host = lambda t: t.cpu().numpy().copy()
    try:
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, joints={})
        runs = {}
        for joints_on in (False, True):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap,
                               joints=dict(tau_max=3.0) if joints_on else None)
            W.replan()
            torch.cuda.synchronize()
            handed = []
            for _ in range(3):
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0)))
                W.replan()
                torch.cuda.synchronize()
                assert (host(W.row) == seg).all()
            mid = dict(traj=host(W.traj), cursor=host(W.cursor), t0=host(W.t0))
            if joints_on:
                mid["joint"], mid["status"] = host(W.joint_traj), host(W.joint_status)
                mid["rows"] = [W.joint_rows(b) for b in range(B)]
            last = dict(nodes=host(W.nodes), t0=host(W.t0))
            W.finish()
            torch.cuda.synchronize()
            end = dict(traj=host(W.traj), cursor=host(W.cursor), t0=host(W.t0))
            if joints_on:
                end["rows"] = [W.joint_rows(b) for b in range(B)]
            else:
                assert W.joint_traj is None
                with pytest.raises(RuntimeError):
                    W.joint_rows(0)
            runs[joints_on] = (handed, mid, last, end)
        (_, mid0, _, end0), (handed, mid, last, end) = runs[False], runs[True]
        for a, b in ((mid0, mid), (end0, end)):                             # the joint kernel only reads the cursor and the clock
            assert np.array_equal(bits(a["traj"]), bits(b["traj"])) and np.array_equal(a["cursor"], b["cursor"])
            assert np.array_equal(bits(a["t0"]), bits(b["t0"]))
        assert (mid["cursor"] == 3 * seg).all() and 3 * seg > cap
        p = capi.joint_params(hz=1000.0, n_rows=seg, tau_max=3.0)
        tables = [P.joint_rows(h["nodes"], h["t0"], p) for h in handed]
        for b in range(B):
            want = np.concatenate([t[0][b] for t in tables])[-cap:]
            want_st = np.concatenate([t[1][b] for t in tables])[-cap:]
            rows, st = mid["rows"][b]
            assert rows.shape == (cap, 37) and np.array_equal(bits(rows), bits(want)) and np.array_equal(st, want_st)
            # row for row with the CSV ring: the same time stamps
            assert np.array_equal(bits(rows[:, 0]), bits(ring_rows(mid["traj"][b], mid["cursor"][b])[:, 0]))
        p = capi.joint_params(hz=1000.0, n_rows=5001, tau_max=3.0)
        full, full_st = P.joint_rows(last["nodes"], last["t0"], p)
        for b in range(B):
            rows, st = end["rows"][b]
            assert np.array_equal(bits(rows), bits(full[b, -cap:])) and np.array_equal(st, full_st[b, -cap:])
            assert np.array_equal(bits(rows[:, 0]), bits(ring_rows(end["traj"][b], end["cursor"][b])[:, 0]))
    finally:
        P.close()


def test_host_form_ring_mode_and_argument_checks(case):
    from qtos_amd import capi
    cap = 300
    ring, st = np.full((1, cap, 37), -7.5), np.full((1, cap), -7, np.int32)
    p = capi.joint_params(hz=HZ, first_row=40, n_rows=200, capacity=cap, tau_max=0.0)
    out, ost = case.P.joint_rows(case.nodes, case.t0, p, out=ring, status=st, cursor=np.array([250], np.int64))
    k = (250 + np.arange(200)) % cap
    assert np.array_equal(bits(out[0, k]), bits(case.rows[0, 40:240])) and np.array_equal(ost[0, k], case.status[0, 40:240])
    rest = np.setdiff1d(np.arange(cap), k)
    assert (out[0, rest] == -7.5).all() and (ost[0, rest] == -7).all() and (ring == -7.5).all()
    many, _ = case.P.joint_rows(case.nodes, case.t0, p, n_rows=np.array([10 ** 6], np.int32), out=ring, status=st, cursor=np.array([-5], np.int64))
    k = (-5 + np.arange(cap)) % cap                                           # a count beyond the ring is clamped to it
    assert np.array_equal(bits(many[0, k]), bits(case.rows[0, 40:40 + cap]))

    def call(**kw):
        a = dict(h=case.P.h, b=1, s=p, nodes=case.nodes, t0=case.t0, cur=np.array([0], np.int64), qm=None, qdm=None, out=ring.copy(), st=st.copy())
        a.update(kw)
        return case.P.lib.qtos_joint_rows(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]),
                                          None, None, None if a["cur"] is None else a["cur"].ctypes.data_as(C.POINTER(C.c_longlong)),
                                          capi._dp(a["qm"]), capi._dp(a["qdm"]), capi._dp(a["out"]), capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            setattr(s, key, v)
        return s
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null t0": call(t0=None), "null out": call(out=None), "null status": call(st=None), "ring without cursor": call(cur=None),
           "capacity < 0": call(s=params(capacity=-1)), "table without rows": call(s=params(capacity=0, n_rows=0)),
           "first_row -1": call(s=params(first_row=-1)), "first_row 1000001": call(s=params(first_row=1000001)),
           "n_rows < 0": call(s=params(n_rows=-1)), "q_mes alone": call(qm=np.zeros((1, 12))), "l_upper 0": call(s=params(l_upper=0.0))}
    assert all(v == -1 for v in got.values()), got
    assert call() == 0 and call(s=params(first_row=1000000)) == 0


def test_joint_rows_from_plain_c(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "joint_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "joint_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_joint_rows=%d joint_null=-1 joint_device_null=-1" % C.sizeof(capi.QtosJointRows)
    assert lines[1] == "bad_args=" + ",".join(["-1"] * 8)
    assert lines[2] == "plan rc=0 status=0,0"
    kv = dict(t.split("=") for t in lines[3].replace("sample rc", "sample_rc").replace("joint rc", "joint_rc").split())
    assert int(kv["sample_rc"]) == 0 and int(kv["joint_rc"]) == 0 and int(kv["stamp_mismatches"]) == 0
    assert lines[4] == "tick rc=0 mismatches=0 clipped=12"
