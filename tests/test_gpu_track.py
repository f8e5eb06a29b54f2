"""The track kernel on the MI355X (pytest -m gpu): k_track against the longdouble statement of the rule (qtos_amd/tracking.py), its
errors and running totals against float64 numpy on its own columns, both delay rules, carried accumulators, the tick, the ring,
a non-default stream, the host form, the calls from plain C and the track ring of ShiftedWindows against table-mode rows.

Shapes.  TILE = 512 rows is the multi-wave tile.  A case is one plan (the golden walk, a trot, the exp_5 step whose base pitches:
three planners, because a planner has one gait's layout) with B = 3 windows of it at 200 Hz, each with a clock and a seeded
perturbation of 1e-3 of its own on the measured state (the planned pose and k_joint_rows' own angles); n_rows = 2 TILE + 37, two
full tiles and a partial one with rows past the horizon; the per-window counts are 0, exactly TILE and the full count.

Accuracy gates.  The feet (and in quaternion mode the Euler columns) are held to the longdouble statement at the larger of 8 x
the float64 numpy floor measured here and a bound propagated from the device math library's errors, capped at 1e-12; as
tests/test_gpu_joints.py states, no document with ROCm's ulp figures is installed next to the compiler, so 4 ulp are ASSUMED for
each of sqrt, sin, cos, atan2 and asin.  With u = 2^-53 (one ulp of v is at most 2 u |v|):

  chain    the sines and cosines of q1, q2, q2 + q3: 8 u each, and 5 u for the rounded sum q2 + q3 (|q| <= 2.4): x and h, sums of
           two products with the links of 0.16 m, are off by 2 x 0.16 x 13 u + 1 u of their own roundings: 5.2 u m; p_y and p_z add
           8 u (|lateral| + h) <= 3 u and 1 u of roundings: 9.2 u m; p_x + p_y + p_z: 24 u m
  R        Euler mode: an entry is at most two products of three sines / cosines: 2 x (24 u + 3 u) + u = 55 u.  Quaternion mode:
           the norm's sqrt and the division leave 12 u on a component, a product of two has 25 u, an entry 2 (a b +- c d) with
           |a b| + |c d| <= 1 about 55 u as well
  feet     com + R p with |p|_1 <= 0.9 m: 55 u x 0.9 + 24 u + 12 u for the three products and three sums: 86 u m, taken as 128 u m
  Euler    quaternion mode, |pitch| <= 1.2: atan2 of two entries 55 u off at a radius of cos(pitch) >= 0.36 is 216 u off, and 4 ulp
           of a result below pi are 25 u: 241 u; asin: 55 u / 0.36 + 10 u = 163 u: taken as 256 u rad
The errors (columns 19 .. 23) are held to the float64 formula on the kernel's own columns within 4 units in the last place: the
sqrt assumption above.  The totals, the counters and the status are exact.  Measured on an MI355X (profiles/track_accuracy.json):
see DESIGN.md section 6."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_gv

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LD, F64 = np.longdouble, np.float64
U = 2.0 ** -53
TILE = 512
HZ, N_ROWS = 200.0, 2 * TILE + 37
CAP = 1e-12
FEET_BOUND, EULER_BOUND = 128 * U, 256 * U
B = 3
COUNTS = np.array([0, TILE, N_ROWS], np.int32)
T0 = np.array([3.756, 0.0, 11.25])
COUNT_IN = np.array([[5, 2], [0, 0], [1, 0]], np.int64)          # (window 2 has one call behind it: with delay TILE + 1 the skipped
TOTAL_IN = np.array([[1.5, 2.5], [0.0, 0.0], [0.25, 0.5]])       # call of the reference rule is the first row of its second tile)
LLP = C.POINTER(C.c_longlong)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def record(name, entry):
    print("track accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_TRACK_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def quat_of(euler):
    """(x, y, z, w) of Rz(yaw) Ry(pitch) Rx(roll), float64."""
    e = np.asarray(euler, F64)
    sr, cr, sp_, cp, sy, cy = (f(e[..., i] / 2) for i in range(3) for f in (np.sin, np.cos))
    return np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], -1)


class Case:
    """One plan: its planner, nodes, the measured tables of B windows, the kernel's base result (reference rule, delay 3, goal_x) and
    the statement's rows in longdouble and float64."""

    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, tracking, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name = name
        cfg = PlannerConfig.reference_compat(gait="trot") if name == "trot" else PlannerConfig.reference_compat()
        self.P = Planner(cfg, max_batch=8)
        if name == "walk":
            nodes = np.array(load_gv("gv1")["x"])[None]
        elif name == "trot":
            start, goal = workloads.flat_goals(1, seed=11)
            nodes, status, _, _ = self.P.plan(start, goal)
            assert status[0] == 0
        else:                                                   # a step onto the ledges of exp_5: the base pitches
            hxy, cell = workloads.exp5_terrain()
            self.P.set_heightfields(hxy, cell)
            start, goal = workloads.step_goals(1, seed=1, terrain=(hxy, cell))
            nodes, status, _, _ = self.P.plan(start, goal)
        self.nodes = np.repeat(nodes, B, axis=0)
        self.L = sp.layout(cfg)
        self.sample = self.P.sample(self.nodes, T0, hz=HZ, n_rows=N_ROWS)                  # the plan's rows, per window's clock
        joint, _ = self.P.joint_rows(nodes, T0[:1], capi.joint_params(hz=HZ, n_rows=N_ROWS, tau_max=0.0))
        rng = np.random.default_rng(41)
        on_plan = np.concatenate([self.sample[0, :, 1:7], joint[0, :, 1:13]], 1)
        self.meas = on_plan[None] + 1e-3 * rng.standard_normal((B, N_ROWS, 18))
        self.meas.setflags(write=False)
        self.goal_x = np.array([np.median(self.meas[b, :max(int(COUNTS[b]), 1), 0]) for b in range(B)])   # about half of a window's rows reach it
        self.rows, self.status, self.count, self.total = self.track(capi.track_params(hz=HZ, n_rows=N_ROWS, delay=3))
        self.want = {}
        for dt in (LD, F64):
            p = tracking.TrackParams(delay=3)
            self.want[dt] = [tracking.track_rows(self.L, self.nodes[b], T0[b], HZ, 0, int(COUNTS[b]), self.meas[b], p, tuple(COUNT_IN[b]),
                                                 tuple(TOTAL_IN[b]), self.goal_x[b], dt) for b in range(B)]

    def track(self, params, meas=None, **kw):
        """The base call: per-window counts, accumulators that stand, goal_x, out and status pre-filled."""
        args = dict(n_rows=COUNTS, goal_x=self.goal_x, count=COUNT_IN, total=TOTAL_IN, out=np.full((B, N_ROWS, 26), -7.5),
                    status=np.full((B, N_ROWS), -7, np.int32))
        args.update(kw)
        return self.P.track(self.nodes, T0, self.meas if meas is None else meas, params, **args)


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


def test_time_stamps_untouched_rows_and_kept_accumulators(case):
    assert case.rows.shape == (B, N_ROWS, 26) and case.status.dtype == np.int32 and case.count.dtype == np.int64
    assert N_ROWS > 2 * TILE and (N_ROWS - 1) / HZ > case.L.T                           # a partial third tile, rows past the horizon
    for b in range(B):
        n = int(COUNTS[b])
        assert np.array_equal(bits(case.rows[b, :n, 0]), bits(case.sample[b, :n, 0]))   # qtos_sample_csv's time stamps, to the bit
        assert (case.rows[b, n:] == -7.5).all() and (case.status[b, n:] == -7).all()    # rows behind a window's count are untouched
    assert np.array_equal(case.count[0], COUNT_IN[0]) and np.array_equal(bits(case.total[0]), bits(TOTAL_IN[0]))
    assert case.count[1:, 0].tolist() == [TILE, 1 + N_ROWS]
    if case.name == "exp5":
        assert np.abs(case.sample[0, :, 5]).max() > 1e-3                                # the base does pitch


def feet_entry(got, want_ld, want_64):
    floor = float(np.abs(want_64[:, 7:19].astype(LD) - want_ld[:, 7:19]).max())
    return dict(floor=floor, gate=min(max(8 * floor, FEET_BOUND), CAP), error=float(np.abs(got[:, 7:19].astype(LD) - want_ld[:, 7:19]).max()))


def test_pose_columns(case):
    entry = {}
    for b in (1, 2):
        n = int(COUNTS[b])
        got = case.rows[b, :n]
        assert np.array_equal(bits(got[:, 1:7]), bits(case.meas[b, :n, 0:6]))            # CoM and Euler columns: the inputs, to the bit
        entry["window%d" % b] = feet_entry(got, case.want[LD][b][0], case.want[F64][b][0])
    record("feet %s" % case.name, entry)
    for v in entry.values():
        assert v["error"] <= v["gate"], (case.name, v)


def test_quaternion_mode(case):
    from qtos_amd import capi, tracking
    n = N_ROWS
    meas = np.zeros((B, n, 19))
    meas[:, :, 0:3], meas[:, :, 7:19] = case.meas[:, :, 0:3], case.meas[:, :, 6:18]
    meas[:, :, 3:7] = quat_of(case.meas[:, :, 3:6]) * 1.7                               # (not normalised)
    meas[2, 700, 3:7] = (0, 3, 0, 3)                                                    # pitch = pi / 2: the clip acts
    rows, status, _, _ = case.track(capi.track_params(hz=HZ, n_rows=n, delay=3, quaternion=True), meas)
    p = tracking.TrackParams(delay=3, quaternion=True)
    entry = {}
    for b in (1, 2):
        m = int(COUNTS[b])
        w_ld, st_ld, _, _ = tracking.track_rows(case.L, case.nodes[b], T0[b], HZ, 0, m, meas[b], p, tuple(COUNT_IN[b]), tuple(TOTAL_IN[b]),
                                                case.goal_x[b], LD)
        w_64, st_64, _, _ = tracking.track_rows(case.L, case.nodes[b], T0[b], HZ, 0, m, meas[b], p, tuple(COUNT_IN[b]), tuple(TOTAL_IN[b]),
                                                case.goal_x[b], F64)
        got = rows[b, :m]
        ok = np.ones(m, bool)
        if b == 2:
            ok[700] = False
            assert status[2, 700] & tracking.GIMBAL and st_64[700] & tracking.GIMBAL and abs(got[700, 5] - np.pi / 2) < 1e-7
        assert np.array_equal(status[b, :m][ok], st_64[ok]) and (status[b, :m][ok] & tracking.GIMBAL == 0).all()
        assert np.array_equal(bits(got[:, 1:4]), bits(meas[b, :m, 0:3]))
        assert float(np.abs(w_ld[ok, 5]).max()) <= 1.2
        e = feet_entry(got[ok], w_ld[ok], w_64[ok])
        floor = float(np.abs(w_64[ok, 4:7].astype(LD) - w_ld[ok, 4:7]).max())
        e.update(euler_floor=floor, euler_gate=min(max(8 * floor, EULER_BOUND), CAP),
                 euler_error=float(np.abs(got[ok, 4:7].astype(LD) - w_ld[ok, 4:7]).max()))
        entry["window%d" % b] = e
    record("quaternion %s" % case.name, entry)
    for v in entry.values():
        assert v["error"] <= v["gate"] and v["euler_error"] <= v["euler_gate"], (case.name, v)


def test_errors_are_the_float64_formula_on_the_kernels_own_columns(case):
    from qtos_amd import tracking
    worst = 0.0
    for b in (1, 2):
        n = int(COUNTS[b])
        want = tracking.errors(case.sample[b, :n], case.rows[b, :n, 1:19])
        assert want.dtype == F64
        worst = max(worst, float((np.abs(case.rows[b, :n, 19:24] - want) / np.spacing(want)).max()))
    record("errors %s" % case.name, dict(worst_units_in_the_last_place=worst))
    assert worst <= 4


@pytest.mark.parametrize("rule", ["reference", "clean"])
@pytest.mark.parametrize("delay", [0, 3, TILE + 1])
def test_totals_counters_and_status_are_exact(case, rule, delay):
    from qtos_amd import capi, tracking
    if (rule, delay) == ("reference", 3):
        rows, status, count, total = case.rows, case.status, case.count, case.total
    else:
        rows, status, count, total = case.track(capi.track_params(hz=HZ, n_rows=N_ROWS, delay=delay, rule=rule))
    p = tracking.TrackParams(delay=delay, rule=rule)
    for b in range(B):
        n = int(COUNTS[b])
        assert np.array_equal(bits(rows[b, :n, :24]), bits(case.rows[b, :n, :24]))        # the pose and the errors do not depend on the rule
        flags, run, cnt, tot = tracking.accumulate(rows[b, :n, 19:24], tuple(COUNT_IN[b]), tuple(TOTAL_IN[b]), p)
        assert np.array_equal(bits(rows[b, :n, 24:26]), bits(run))
        assert tuple(count[b]) == cnt and np.array_equal(bits(total[b]), bits(np.array(tot)))
        want = np.where(flags, tracking.RECORDED, 0) | np.where(case.meas[b, :n, 0] >= case.goal_x[b], tracking.REACHED, 0)
        assert np.array_equal(status[b, :n], want.astype(np.int32))
        if n:
            assert 0 < (status[b, :n] & tracking.REACHED != 0).sum() < n
    if rule == "reference" and delay == TILE + 1:                                        # the skipped call is the first row of window 2's second tile
        assert status[2, TILE - 1] & 1 and not status[2, TILE] & 1 and status[2, TILE + 1] & 1
    free = case.track(capi.track_params(hz=HZ, n_rows=N_ROWS, delay=delay, rule=rule), goal_x=None)[1]
    assert (free[2] & tracking.REACHED == 0).all()                                        # without goal_x the bit is never set


def test_two_launches_with_carried_accumulators_are_one(case):
    from qtos_amd import capi
    cut = 600
    b = 2
    one = (case.rows[b:b + 1], case.status[b:b + 1], case.count[b:b + 1], case.total[b:b + 1])
    nodes, t0, goal = case.nodes[b:b + 1], T0[b:b + 1], case.goal_x[b:b + 1]
    first = case.P.track(nodes, t0, case.meas[b:b + 1, :cut], capi.track_params(hz=HZ, n_rows=cut, delay=3), goal_x=goal,
                         count=COUNT_IN[b:b + 1], total=TOTAL_IN[b:b + 1])
    second = case.P.track(nodes, t0, case.meas[b:b + 1, cut:], capi.track_params(hz=HZ, first_row=cut, n_rows=N_ROWS - cut, delay=3),
                          goal_x=goal, count=first[2], total=first[3])
    assert np.array_equal(bits(np.concatenate([first[0], second[0]], 1)), bits(one[0]))
    assert np.array_equal(np.concatenate([first[1], second[1]], 1), one[1])
    assert np.array_equal(second[2], one[2]) and np.array_equal(bits(second[3]), bits(one[3]))


def test_tick_of_five_robots(case):
    """B = 5, one row each at a row index of its own: the one-wave instantiation's rows are the table's rows, to the bit."""
    from qtos_amd import capi, tracking
    n = 5
    first = np.array([0, 1, TILE - 1, TILE, N_ROWS - 1], np.int32)
    nodes, t0 = np.repeat(case.nodes[2:3], n, axis=0), np.repeat(T0[2:3], n)
    meas = case.meas[2, first][:, None, :]
    goal_x = meas[:, 0, 0] + np.array([0.01, -0.01, 0.01, -0.01, 0.01])                    # robots 1 and 3 have reached theirs
    count_in = np.stack([np.arange(n) + 10, np.arange(n)], 1).astype(np.int64)
    total_in = np.stack([0.5 + np.arange(n), 1.5 + np.arange(n)], 1)
    p = capi.track_params(hz=HZ, n_rows=1, delay=11, rule="clean")                         # robot 0 (call 11) is not recorded yet
    rows, status, count, total = case.P.track(nodes, t0, meas, p, first_row=first, goal_x=goal_x, count=count_in, total=total_in)
    assert rows.shape == (n, 1, 26) and status.shape == (n, 1)
    assert np.array_equal(bits(rows[:, 0, :24]), bits(case.rows[2, first, :24]))
    assert status[:, 0].tolist() == [0, 3, 1, 3, 1]
    e = rows[:, 0, 19:24]
    want_com = np.where(np.arange(n) > 0, total_in[:, 0] + e[:, 0], total_in[:, 0])
    want_feet = np.where(np.arange(n) > 0, (((total_in[:, 1] + e[:, 1]) + e[:, 2]) + e[:, 3]) + e[:, 4], total_in[:, 1])
    assert np.array_equal(bits(rows[:, 0, 24]), bits(want_com)) and np.array_equal(bits(rows[:, 0, 25]), bits(want_feet))
    assert np.array_equal(bits(total), bits(rows[:, 0, 24:26]))
    assert count[:, 0].tolist() == (count_in[:, 0] + 1).tolist() and count[:, 1].tolist() == [0, 2, 3, 4, 5]
    # a full wave of the one-wave kernel, and one row more (the 512-lane kernel): the table's rows, to the bit
    tp = tracking.TrackParams(delay=3)
    for m in (64, 65):
        part = case.P.track(case.nodes[2:3], T0[2:3], case.meas[2:3, 100:100 + m], capi.track_params(hz=HZ, first_row=100, n_rows=m, delay=3))
        assert np.array_equal(bits(part[0][0, :, :24]), bits(case.rows[2, 100:100 + m, :24]))
        flags, run, cnt, tot = tracking.accumulate(part[0][0, :, 19:24], (0, 0), (0.0, 0.0), tp)
        assert np.array_equal(bits(part[0][0, :, 24:26]), bits(run)) and tuple(part[2][0]) == cnt
        assert np.array_equal(bits(part[3][0]), bits(np.array(tot))) and np.array_equal(part[1][0] & 1, flags.astype(np.int32))


def test_ring_mode_is_the_table(case):
    """Capacity 300, two appends of 200 rows, the second wraps: the ring's rows are the table-mode rows of the same row numbers."""
    from qtos_amd import capi
    from qtos_amd.stitcher import ring_rows
    cap, seg, b = 300, 200, 2
    nodes, t0, goal = case.nodes[b:b + 1], T0[b:b + 1], case.goal_x[b:b + 1]
    table = case.P.track(nodes, t0, case.meas[b:b + 1, :2 * seg], capi.track_params(hz=HZ, n_rows=2 * seg, delay=3), goal_x=goal)
    ring, st, ring_meas = np.full((1, cap, 26), -7.5), np.full((1, cap), -7, np.int32), np.full((1, cap, 18), np.nan)
    cursor, count, total = 0, None, None
    for i in range(2):
        at = (cursor + np.arange(seg)) % cap
        ring_meas[0, at] = case.meas[b, i * seg:(i + 1) * seg]
        p = capi.track_params(hz=HZ, first_row=i * seg, n_rows=seg, capacity=cap, delay=3)
        ring, st, count, total = case.P.track(nodes, t0, ring_meas, p, cursor=np.array([cursor], np.int64), goal_x=goal, count=count,
                                              total=total, out=ring, status=st)
        if i == 0:
            assert (ring[0, seg:] == -7.5).all() and (st[0, seg:] == -7).all()
        cursor += seg
    assert np.array_equal(bits(ring_rows(ring[0], cursor)), bits(table[0][0, -cap:]))
    assert np.array_equal(ring_rows(st[0], cursor), table[1][0, -cap:])
    assert np.array_equal(count, table[2]) and np.array_equal(bits(total), bits(table[3]))


def test_device_form_on_a_held_up_stream_is_the_host_form(case):
    import torch
    from qtos_amd import capi
    dev = torch.device("cuda", 0)
    p = capi.track_params(hz=HZ, n_rows=N_ROWS, delay=3)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0, d_n = torch.as_tensor(T0, **f64), torch.as_tensor(COUNTS, device=dev)
    d_meas, d_goal = torch.as_tensor(np.array(case.meas), **f64), torch.as_tensor(case.goal_x, **f64)
    src = torch.as_tensor(case.nodes, **f64)
    side = torch.cuda.Stream(dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)              # (elementwise work: holds the stream up, loads no BLAS library)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        out, st = torch.full((B, N_ROWS, 26), -7.5, **f64), torch.full((B, N_ROWS), -7, dtype=torch.int32, device=dev)
        count, total = torch.as_tensor(COUNT_IN, device=dev), torch.as_tensor(TOTAL_IN, **f64)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if stream is side:
                for _ in range(50):
                    busy.mul_(1.0001).clamp_(0.0, 1.0)
            d_nodes = src + 0.0
            rc = case.P.lib.qtos_track_device(case.P.h, B, C.byref(p), d_nodes.data_ptr(), d_t0.data_ptr(), None, d_n.data_ptr(), None,
                                              d_meas.data_ptr(), d_goal.data_ptr(), count.data_ptr(), total.data_ptr(), out.data_ptr(),
                                              st.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert rc == 0, case.P.lib.qtos_last_error(case.P.h)
        stream.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(case.rows)) and np.array_equal(st.cpu().numpy(), case.status)
        assert np.array_equal(count.cpu().numpy(), case.count) and np.array_equal(bits(total.cpu().numpy()), bits(case.total))
    torch.cuda.synchronize()


def test_argument_checks(case):
    from qtos_amd import capi
    cap = 300
    p = capi.track_params(hz=HZ, first_row=40, n_rows=200, capacity=cap, delay=3)
    ring, st, meas = np.zeros((1, cap, 26)), np.zeros((1, cap), np.int32), np.zeros((1, cap, 18))
    count, total = np.zeros((1, 2), np.int64), np.zeros((1, 2))

    def call(**kw):
        a = dict(h=case.P.h, b=1, s=p, nodes=case.nodes[:1], t0=T0[:1], cur=np.array([0], np.int64), meas=meas, count=count.copy(),
                 total=total.copy(), out=ring.copy(), st=st.copy())
        a.update(kw)
        ll = lambda v: None if v is None else v.ctypes.data_as(LLP)
        return case.P.lib.qtos_track(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]),
                                     None, None, ll(a["cur"]), capi._dp(a["meas"]), None, ll(a["count"]), capi._dp(a["total"]),
                                     capi._dp(a["out"]), capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            setattr(s, key, v)
        return s
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null t0": call(t0=None), "null meas": call(meas=None), "null count": call(count=None), "null total": call(total=None),
           "null out": call(out=None), "null status": call(st=None), "ring without cursor": call(cur=None),
           "capacity < 0": call(s=params(capacity=-1)), "table without rows": call(s=params(capacity=0, n_rows=0)),
           "first_row -1": call(s=params(first_row=-1)), "first_row 1000001": call(s=params(first_row=1000001)),
           "n_rows < 0": call(s=params(n_rows=-1)), "delay < 0": call(s=params(delay=-1)), "l_upper 0": call(s=params(l_upper=0.0)),
           "l_lower 0": call(s=params(l_lower=0.0))}
    assert all(v == -1 for v in got.values()), got
    assert call() == 0 and call(s=params(first_row=1000000)) == 0 and call(s=params(delay=0)) == 0


def test_track_from_plain_c(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "track_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "track_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_track=%d track_null=-1 track_device_null=-1" % C.sizeof(capi.QtosTrack)
    assert lines[1] == "bad_args=" + ",".join(["-1"] * 9)
    assert lines[2] == "plan rc=0 status=0,0"
    kv = dict(t.split("=") for t in lines[3].replace("track rc", "track_rc").split())
    assert int(kv["track_rc"]) == 0 and int(kv["mismatches"]) == 0 and int(kv["clean_rows"]) > 0
    assert float(kv["largest_error"]) < 1e-12                      # a robot on its plan: rounding only
    assert lines[4].startswith("totals com=") and lines[4].endswith("recorded=998,998")
    assert lines[5] == "tick rc=0 mismatches=0"


def test_track_ring_of_shifted_windows_is_the_table_row_for_row():
    """Capacity 700, three segments of 300 rows, then finish(): every track ring row is the table-mode row of the same plan and
    index with the accumulators carried from segment to segment, to the bit; the measured ring is filled from the joint ring by a
    torch op on the windows' stream; the CSV ring, the cursor and the clock are what they are without `track`."""
    import torch
    from qtos_amd import capi, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    nb, cap, seg = 4, 700, 300
    start, goal = workloads.flat_goals(nb, seed=7)
    P = Planner(PlannerConfig.knots100(gait="trot"), max_batch=nb)
    host = lambda t: t.cpu().numpy().copy()
    pose = np.array([[0.1 * b, 0.01 * b, 0.24, 0.01, -0.02 * b, 0.03] for b in range(nb)])
    goal_x = np.array([0.05, 0.05, 0.15, 0.35])                   # windows 0 and 3 stand behind their goal, 1 and 2 have reached it

    def fill(W):          # the robot stands at `pose` with the commanded joint angles: on the windows' stream, behind the joint rows
        assert torch.cuda.current_stream(W.dev) == W.stream
        W.meas_traj[:, :, 0:6] = torch.as_tensor(pose, dtype=torch.float64, device=W.dev)[:, None, :]
        W.meas_traj[:, :, 6:18] = W.joint_traj[:, :, 1:13]
    try:
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, track={})
        runs = {}
        for on in (False, True):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(tau_max=3.0),
                               track=dict(delay=3, goal_x=goal_x, fill=fill) if on else None, stream=torch.cuda.Stream())
            if not on:
                assert W.track_traj is None and not hasattr(W, "meas_traj") and not hasattr(W, "track_total")

                def never(*a):
                    raise AssertionError("a track call was queued")
                W._track_rows = never
                with pytest.raises(RuntimeError):
                    W.track_rows(0)
            W.replan()
            torch.cuda.synchronize()
            handed = []
            for _ in range(3):
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0)))
                W.replan()
                torch.cuda.synchronize()
                assert (host(W.row) == seg).all()
            mid = dict(traj=host(W.traj), cursor=host(W.cursor), t0=host(W.t0))
            if on:
                mid["rows"] = [W.track_rows(b) for b in range(nb)]
                mid["count"], mid["total"] = host(W.track_count), host(W.track_total)
            last = dict(nodes=host(W.nodes), t0=host(W.t0))
            W.finish()
            torch.cuda.synchronize()
            end = dict(traj=host(W.traj), cursor=host(W.cursor), t0=host(W.t0))
            if on:
                end["rows"] = [W.track_rows(b) for b in range(nb)]
                end["count"], end["total"] = host(W.track_count), host(W.track_total)
            runs[on] = (handed, mid, last, end)
        (_, mid0, _, end0), (handed, mid, last, end) = runs[False], runs[True]
        for a, b in ((mid0, mid), (end0, end)):                             # the track kernel only reads the cursor and the clock
            assert np.array_equal(bits(a["traj"]), bits(b["traj"])) and np.array_equal(a["cursor"], b["cursor"])
            assert np.array_equal(bits(a["t0"]), bits(b["t0"]))
        assert (mid["cursor"] == 3 * seg).all() and 3 * seg > cap

        def table(h, n, count, total):
            joint, _ = P.joint_rows(h["nodes"], h["t0"], capi.joint_params(hz=1000.0, n_rows=n, tau_max=3.0))
            meas = np.concatenate([np.repeat(pose[:, None, :], n, axis=1), joint[:, :, 1:13]], 2)
            return P.track(h["nodes"], h["t0"], meas, capi.track_params(hz=1000.0, n_rows=n, delay=3), goal_x=goal_x, count=count, total=total)
        count = total = None
        tables = []
        for h in handed:
            tables.append(table(h, seg, count, total))
            count, total = tables[-1][2], tables[-1][3]
        assert np.array_equal(mid["count"], count) and np.array_equal(bits(mid["total"]), bits(total))
        assert (count[:, 0] == 3 * seg).all() and (count[:, 1] == 3 * seg - 3).all()
        for b in range(nb):
            rows, st = mid["rows"][b]
            assert rows.shape == (cap, 26)
            assert np.array_equal(bits(rows), bits(np.concatenate([t[0][b] for t in tables])[-cap:]))
            assert np.array_equal(st, np.concatenate([t[1][b] for t in tables])[-cap:])
            assert ((st & 2) != 0).all() == (b in (1, 2)) and ((st & 2) != 0).any() == (b in (1, 2))
        full = table(last, 5001, count, total)
        assert np.array_equal(end["count"], full[2]) and np.array_equal(bits(end["total"]), bits(full[3]))
        for b in range(nb):
            rows, st = end["rows"][b]
            assert np.array_equal(bits(rows), bits(full[0][b, -cap:])) and np.array_equal(st, full[1][b, -cap:])
    finally:
        P.close()
