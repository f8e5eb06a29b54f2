"""The feedback hand-over rule in numpy (qtos_amd/feedback.py, what k_start_feedback is held to) on the golden walk
(tests/golden/gv1.npz, PlannerConfig.reference_compat()): gains 0, a robot exactly on its plan, a rigid drift, a base-only offset
that leaves the range-of-motion box, the special cases of the rule, starts the CPU oracle solves, and the C ABI.

Rows.  The hand-over rows below were found with the rule itself: at 1 kHz, measured = the plan's own row r - 1 with the joint
angles of joints.joint_rows, shifted rigidly by D, none of the rows 100, 200, ..., 5000 of gv1 falls back.  STANCE are rows with all
four feet on the ground (the snap moves no z by more than rounding), SWING rows with one foot in the air (the snap puts it down
and says so); row 500 is left out, where the plan asks a leg to reach beyond its length and the robot cannot be on it."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, load_gv

from oracle import splines as sp
from qtos_amd import feedback as F
from qtos_amd import joints as J
from qtos_amd import tracking as T
from qtos_amd.config import PlannerConfig

LD, F64 = np.longdouble, np.float64
HZ = 1000.0
D = np.array([0.010, -0.005, 0.0])
STANCE = (100, 700, 1000, 2000, 2900, 3500)
SWING = ((300, 2), (600, 0), (900, 3), (1200, 1))       # (row, the foot in the air)


@pytest.fixture(scope="module")
def walk():
    """The golden walk: (layout, nodes)."""
    return sp.layout(PlannerConfig.reference_compat()), load_gv("gv1")["x"]


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def handover_start(L, x, r, t0=0.0):
    """What k_handover writes for row r: columns 1 .. 18 of the row and, here, no velocities."""
    return np.concatenate([T.plan_positions(L, x, t0, HZ, r, 1, F64)[0, 1:19], np.zeros(6)])


def on_plan(L, x, k, t0=0.0, dtype=LD):
    """The measured row of a robot exactly on plan row k: the planned base pose and joints.joint_rows' angles."""
    plan = T.plan_positions(L, x, t0, HZ, k, 1, dtype)
    rows, status = J.joint_rows(L, x, t0, HZ, k, 1, J.JointParams(), dtype=dtype)
    assert status[0] == 0
    return np.concatenate([plan[0, 1:7], rows[0, 1:13]])


def table(r, k, row, dtype=LD):
    """A table of r measured rows, NaN but row k."""
    m = np.full((r, len(row)), np.nan, dtype)
    m[k] = row
    return m


def test_gains_zero_change_nothing_and_each_gain_touches_its_own_columns(walk):
    L, x = walk
    r = 2000
    meas = on_plan(L, x, r - 1, dtype=F64)
    meas[0:18] += 1e-3 * np.random.default_rng(5).standard_normal(18)
    start = handover_start(L, x, r)
    start[18:24] = 0.1 * np.arange(1, 7)
    start[3] = -0.0                                                                  # (a sum with 0 would make it +0)
    for dt in (F64, LD):
        p = F.FeedbackParams(n_rows=r, gain_pos=0, gain_ang=0, gain_foot=0)
        out, goal, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas, dt), p, start, goal_step=[0.3, 0.1, 9.0], dtype=dt)
        assert st == 0 and out.dtype == dt and np.array_equal(bits(out), bits(start))
        assert np.abs(err).max() > 1e-4 and goal[0] == dt(start[0]) + dt(0.3) and goal[1] == dt(start[1]) + dt(0.1) and goal.shape == (2,)
    cols = dict(gain_pos=range(0, 3), gain_ang=range(3, 6), gain_foot=range(6, 18))
    for name, own in cols.items():
        kw = dict(gain_pos=0, gain_ang=0, gain_foot=0, snap=False)
        kw[name] = 0.5
        out, _, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas, F64), F.FeedbackParams(n_rows=r, **kw), start, dtype=F64)
        assert st == F.CORRECTED
        for i in range(24):
            if i in own:
                assert out[i] == start[i] + 0.5 * err[i] and out[i] != start[i]
            else:
                assert bits(out[i]) == bits(start[i])


@pytest.mark.parametrize("r", STANCE)
def test_robot_exactly_on_the_plan(walk, r):
    """|e| <= 1e-15 and the correction moves the start by no more.  The snap is a step of its own: it puts every stance foot's z on
    the terrain, and the golden plan's own z are up to 1.2e-13 m off it (its solver's residual, not an error of the robot), so
    with the snap the z columns are the terrain's to the bit and the other columns are held to 1e-15."""
    L, x = walk
    start = handover_start(L, x, r)
    meas = table(r, r - 1, on_plan(L, x, r - 1))
    out, _, err, st = F.start_feedback(L, x, 0.0, r, meas, F.FeedbackParams(n_rows=r, snap=False), start, dtype=LD)
    print("on the plan, row %d: |e| %.2e, start moves %.2e" % (r, float(np.abs(err).max()), float(np.abs(out - start).max())))
    assert st == F.CORRECTED and float(np.abs(err).max()) <= 1e-15 and float(np.abs(out - start).max()) <= 1e-15
    snap, _, err2, st = F.start_feedback(L, x, 0.0, r, meas, F.FeedbackParams(n_rows=r), start, dtype=LD)
    z = np.zeros(24, bool)
    z[8:18:3] = True
    assert st == F.CORRECTED and np.array_equal(err2, err) and np.array_equal(snap[~z], out[~z]) and (snap[z] == 0).all()
    assert float(np.abs(start[z]).max()) <= 1.2e-13


@pytest.mark.parametrize("r,gain", [(r, g) for r in STANCE + tuple(s[0] for s in SWING) for g in (1.0, 0.5)])
def test_rigid_drift(walk, r, gain):
    L, x = walk
    start = handover_start(L, x, r)
    meas = on_plan(L, x, r - 1)
    meas[0:3] += D.astype(LD)
    p = F.FeedbackParams(n_rows=r, gain_pos=gain, gain_ang=gain, gain_foot=gain)
    out, goal, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), p, start, goal_step=[0.2, 0.0, 0.0], dtype=LD)
    assert not st & F.FALLBACK and st & F.CORRECTED and not st & F.CLIPPED                  # the cap: no fallback
    want = LD(gain) * D.astype(LD)
    assert float(np.abs(out[0:3] - start[0:3] - want).max()) <= 1e-15
    for f in range(4):
        assert float(np.abs(out[6 + 3 * f:8 + 3 * f] - start[6 + 3 * f:8 + 3 * f] - want[0:2]).max()) <= 1e-15
        assert out[8 + 3 * f] == 0                                                         # the terrain's: flat ground
    assert float(np.abs(out[3:6] - start[3:6]).max()) <= 1e-15 and np.array_equal(out[18:24], start[18:24])
    air = dict(SWING).get(r)
    assert st >> 6 == (0 if air is None else 1 << air)                                     # a foot in the air is put down
    assert float(np.abs(goal - (out[0:2] + np.array([0.2, 0.0], LD))).max()) == 0


def test_base_only_offset_falls_back(walk):
    """The base is measured 0.2 m ahead and the feet where they are planned; with the clips opened and the feet's gain 0 the
    corrected base leaves every foot outside its box."""
    L, x = walk
    r = 2000
    start = handover_start(L, x, r)
    start[18:24] = 0.01 * np.arange(1, 7)
    meas = on_plan(L, x, r - 1)
    meas[0] += LD(0.2)
    kw = dict(n_rows=r, max_pos=1.0, max_ang=1.0, max_foot=1.0, gain_foot=0.0)
    for dt in (F64, LD):
        out, goal, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas, dt), F.FeedbackParams(**kw), start,
                                              goal_step=[0.3, 0.0, 0.0], dtype=dt)
        assert st & F.FALLBACK and not st & F.CORRECTED and not st & F.CLIPPED
        assert np.array_equal(bits(out), bits(start)) and abs(float(err[0]) - 0.2) < 1e-12
        assert goal[0] == dt(start[0]) + dt(0.3)
    # the box is what decides: the same offset within it is taken
    out, _, _, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(gain_pos=0.01, **kw), start, dtype=LD)
    assert st == F.CORRECTED and abs(float(out[0] - start[0]) - 0.002) < 1e-12
    # every foot is outside in x: a box opened by half the offset still falls back, opened by all of it (and in y: the base is turned by 0.29 rad) it does not
    d = np.array(PlannerConfig().max_deviation)
    out, _, _, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(max_deviation=d + [0.1, 0.06, 0], **kw), start, dtype=LD)
    assert st & F.FALLBACK
    out, _, _, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(max_deviation=d + [0.25, 0.06, 0], **kw), start, dtype=LD)
    assert st == F.CORRECTED


def test_clip_bit_and_yaw_wrap(walk):
    L, x = walk
    r = 1000
    start = handover_start(L, x, r)
    meas = on_plan(L, x, r - 1)
    meas[0] += LD(0.08)
    out, _, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r), start, dtype=LD)
    assert st & F.CLIPPED and err[0] == LD(0.05) and float(np.abs(err[6::3] - LD(0.05)).max()) == 0       # the feet ride along
    assert abs(float(out[0] - start[0]) - 0.05) < 1e-15
    # the yaw: planned 3.1, measured -3.1 is +0.083 away, not -6.2
    for dt in (F64, LD):
        assert abs(float(F.wrap_yaw(dt(-3.1) - dt(3.1), dt)) - (2 * math.pi - 6.2)) < 1e-15
        assert F.wrap_yaw(dt(0.25), dt) == dt(0.25) and F.wrap_yaw(dt(-3.0), dt) == dt(-3.0)
    assert float(F.wrap_yaw(F64(-6.2), F64)) == math.remainder(-6.2, 2 * math.pi)
    plan_yaw = float(T.plan_positions(L, x, 0.0, HZ, r - 1, 1, F64)[0, 6])
    meas = on_plan(L, x, r - 1)
    meas[5] = LD(plan_yaw) + LD(2 * math.pi) - LD(0.05)                                # the same heading, 0.05 rad short, a turn on
    p = F.FeedbackParams(n_rows=r, gain_pos=0, gain_foot=0, max_foot=1.0, max_pos=1.0)
    out, _, err, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), p, start, dtype=LD)
    assert abs(float(err[5]) + 0.05) < 1e-15 and not st & F.CLIPPED and abs(float(out[5] - start[5]) + 0.05) < 1e-15


def test_quaternion_input_is_the_euler_input(walk):
    L, x = walk
    r = 2900
    start = handover_start(L, x, r)
    meas = on_plan(L, x, r - 1)
    meas[0:3] += D.astype(LD)
    meas[3:6] += np.array([0.02, -0.03, 0.04], LD)
    e = meas[None, 3:6]
    sr, cr, sp_, cp, sy, cy = (f(e[:, i] / 2) for i in range(3) for f in (np.sin, np.cos))
    quat = np.stack([sr * cp * cy - cr * sp_ * sy, cr * sp_ * cy + sr * cp * sy, cr * cp * sy - sr * sp_ * cy, cr * cp * cy + sr * sp_ * sy], 1)[0]
    mq = np.concatenate([meas[0:3], 1.7 * quat, meas[6:18]])
    a = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r), start, dtype=LD)
    b = F.start_feedback(L, x, 0.0, r, table(r, r - 1, mq), F.FeedbackParams(n_rows=r, quaternion=True), start, dtype=LD)
    assert a[3] == b[3] == F.CORRECTED
    assert float(np.abs(a[0] - b[0]).max()) <= 1e-15 and float(np.abs(a[2] - b[2]).max()) <= 1e-15          # tracking's gate
    with pytest.raises(ValueError):
        F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r, quaternion=True), start, dtype=LD)
    # the pitch clip is carried into the status word
    mq[3:7] = (0, 3, 0, 3)
    st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, mq), F.FeedbackParams(n_rows=r, quaternion=True), start, dtype=LD)[3]
    assert st & F.GIMBAL and st & F.CLIPPED


def test_no_measurement_latency_ring_and_table(walk):
    L, x = walk
    r, first = 700, 2
    start = handover_start(L, x, r)
    p = F.FeedbackParams(n_rows=r, first_row=first)
    out, goal, err, st = F.start_feedback(L, x, 0.0, 0, np.zeros((r, 18)), p, start, goal_step=[0.3, 0, 0], dtype=F64)
    assert st == F.NO_MEASUREMENT and goal is None and np.array_equal(bits(out), bits(start)) and not err.any()
    assert F.measured_row(-3, p) is None and F.measured_row(r + 3, p) is None            # (a place the table of r rows does not hold)
    # which row: r - lat, clamped to the rows the stitch appends, first .. first + r - 1
    assert F.measured_row(r, p) == (r, r - first)                                          # (r - 0 lies within first .. first + r - 1)
    for latency, k in ((0.0, r), (0.0004, r), (0.0006, r - 1), (0.25, r - 250), (0.698, first), (3.0, first)):
        q = F.FeedbackParams(n_rows=r, first_row=first, latency=latency)
        assert F.measured_row(r, q) == (k, k - first), latency
    assert F.lag_rows(F.FeedbackParams(latency=0.0125, hz=200.0)) == 3                    # halves away from zero
    # the row that is picked is the row that is read: every other row is NaN
    lat = F.FeedbackParams(n_rows=r, first_row=first, latency=0.3)
    k, j = F.measured_row(r, lat)
    meas = on_plan(L, x, k)
    meas[0:3] += D.astype(LD)
    one = F.start_feedback(L, x, 0.0, r, table(r, j, meas), lat, start, dtype=LD)
    assert one[3] & F.CORRECTED and abs(float(one[2][0]) - 0.01) < 1e-15
    # the ring picks the same row: (cursor + j) mod capacity, wrapping
    cap = 900
    ring = np.full((cap, 18), np.nan, LD)
    cursor = 5 * cap + 700
    assert cursor % cap + j >= cap                                                        # (it wraps)
    ring[(cursor + j) % cap] = meas
    rp = F.FeedbackParams(capacity=cap, first_row=first, latency=0.3)
    two = F.start_feedback(L, x, 0.0, r, ring, rp, start, cursor=cursor, dtype=LD)
    assert two[3] == one[3] and np.array_equal(one[0], two[0]) and np.array_equal(one[2], two[2])
    assert F.measured_row(cap + 5, F.FeedbackParams(capacity=cap)) is None                # a ring row that was overwritten


def test_snap_bit_on_climb_1_and_zero_filter(walk):
    from qtos_amd import heightfield, workloads
    L, x = walk
    r = 2000
    start = handover_start(L, x, r)
    m = heightfield.build_map([workloads.tile("climb_1"), workloads.tile("climb_1")], 11)
    hxy, cell = heightfield.towr_map(m), heightfield.cell_size(m)
    # climb_1 rises from 0 to 0.065 m at x = 1 of the map: the map is laid so that the ledge starts 5 mm in front of foot FL
    assert heightfield.height_at(hxy, cell, 0.99, 0.0, mode=1) == 0.0 and heightfield.height_at(hxy, cell, 1.01, 0.0, mode=1) == 0.065
    assert hxy[220, 110] == 0.0 and hxy[221, 110] == 0.065
    x0 = float(start[6]) + 0.005 - 220.5 * cell                                        # (nearest cell: cell 221, the ledge's first, starts half a cell early)
    height = F.terrain_lookup(hxy, cell, x0=x0, mode=1)
    up = height(0, start[6] + 0.01, start[7])
    assert height(0, start[6], start[7]) == 0.0 and up >= 0.05
    assert height(7, start[6] + 0.01, start[7]) == up and height(-1, start[6], start[7]) == 0.0         # (one map: every id reads it)
    p = F.FeedbackParams(n_rows=r)
    stay = F.start_feedback(L, x, 0.0, r, table(r, r - 1, on_plan(L, x, r - 1)), p, start, height, dtype=LD)
    assert stay[3] == F.CORRECTED and float(np.abs(stay[0][8::3][:4]).max()) == 0
    meas = on_plan(L, x, r - 1)
    meas[0:3] += D.astype(LD)
    over = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), p, start, height, dtype=LD)
    zs = [height(0, F64(over[0][6 + 3 * f]), F64(over[0][7 + 3 * f])) for f in range(4)]
    assert zs[0] == up and zs[2] == zs[3] == 0.0                                        # the front foot is across, the hind feet are not
    assert over[3] == F.CORRECTED | sum(F.SNAPPED << f for f in range(4) if zs[f] > 0.02)
    assert [float(v) for v in over[0][8:18:3]] == zs
    tol = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r, snap_tol=0.085), start, height, dtype=LD)
    assert tol[3] == F.CORRECTED and tol[0][8] == LD(up)
    off = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r, snap=False), start, height, dtype=LD)
    assert off[3] == F.CORRECTED and abs(float(off[0][8] - start[8])) < 1e-15
    # zero filter: |v| < 1e-4 becomes 0, on the whole vector
    s2 = start.copy()
    s2[18], s2[19] = 5e-5, 2e-4
    small = on_plan(L, x, r - 1)
    small[1] += LD(3e-5) - LD(float(start[1]) - float(T.plan_positions(L, x, 0.0, HZ, r - 1, 1, F64)[0, 2]))
    plain = F.start_feedback(L, x, 0.0, r, table(r, r - 1, small), F.FeedbackParams(n_rows=r), s2, dtype=LD)
    filt = F.start_feedback(L, x, 0.0, r, table(r, r - 1, small), F.FeedbackParams(n_rows=r, zero_filter=True), s2, dtype=LD)
    tiny = np.abs(plain[0]) < LD(1e-4)
    assert tiny[18] and not tiny[19] and tiny[:18].any() and (filt[0][tiny] == 0).all() and np.array_equal(filt[0][~tiny], plain[0][~tiny])


def solve(O, start, goal):
    return O.solve(O.problem(start[0:3], start[3:6], start[6:18].reshape(4, 3), goal, start[18:21], start[21:24]))


def test_corrected_starts_are_solved_by_the_oracle_on_flat_ground(walk, oracle):
    L, x = walk
    for r in (2000, 2900):
        start = handover_start(L, x, r)
        meas = on_plan(L, x, r - 1)
        meas[0:3] += D.astype(LD)
        out, goal, _, st = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r), start,
                                            goal_step=[0.4, 0.0, 0.0], dtype=F64)
        assert st == F.CORRECTED and out.dtype == F64
        xs, info = solve(oracle, out, [goal[0], goal[1], 0.24])
        assert info.status == 0 and oracle.max_violation(xs) <= 1e-4 + 1e-9, (r, info.status)


def test_corrected_start_is_solved_by_the_oracle_on_climb_1():
    """A walk down the ledges of climb_1 (0.065 and 0.05 m under the hind feet, 0.025 m under the front feet, then the ground),
    replanned from a corrected start 1.2 s in."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    cfg = PlannerConfig.reference_compat()
    hxy, cell = workloads.exp5_terrain()                      # tiles climb_2, climb_1: climb_1 is x = 1 .. 3
    O = Oracle(oracle_dict(cfg), height=hxy, hcell=cell)
    height = F.terrain_lookup(hxy, cell, mode=cfg.terrain_mode)
    assert height(0, 1.1, 0.0) == 0.065 and height(0, 1.4, 0.0) == 0.025 and height(0, 1.6, 0.0) == 0.0
    assert height(0, 1.1, 0.0) == O.terrain_height(1.1, 0.0) and height(0, 1.4, 0.1) == O.terrain_height(1.4, 0.1)
    x0 = 1.25
    feet = workloads.NOMINAL_FEET + np.array([x0, 0.0, 0.0])
    fz = np.array([height(0, f[0], f[1]) for f in feet])
    assert fz.tolist() == [0.025, 0.025, 0.065, 0.05]
    first = workloads.rest_start(x0, 0.0, 0.24 + float(fz.mean()), fz)
    xs, info = solve(O, first, [x0 + 0.35, 0.0, 0.24])
    assert info.status == 0
    L = sp.layout(cfg)
    r = 1200
    rows = O.sample(xs, 0.0)
    assert (rows[r, 27:37:3] > 0).sum() == 3                  # a row with a foot in the air: the snap puts it down
    start = handover_start(L, xs, r)
    assert np.array_equal(bits(start[:18]), bits(rows[r, 1:19])) or np.abs(start[:18] - rows[r, 1:19]).max() < 1e-12
    meas = on_plan(L, xs, r - 1)
    meas[0:3] += D.astype(LD)
    out, goal, _, st = F.start_feedback(L, xs, 0.0, r, table(r, r - 1, meas), F.FeedbackParams(n_rows=r), start, height,
                                        goal_step=[0.35, 0.0, 0.0], dtype=F64)
    assert st & F.CORRECTED and not st & F.FALLBACK
    for f in range(4):
        assert out[8 + 3 * f] == height(0, out[6 + 3 * f], out[7 + 3 * f])
    x2, info2 = solve(O, out, [goal[0], goal[1], 0.24])
    assert info2.status == 0 and O.max_violation(x2) <= 1e-4 + 1e-9


def test_abi_exports_struct_and_params(hip_lib, tmp_path):
    from qtos_amd import capi
    for name in ("qtos_start_feedback", "qtos_start_feedback_device"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    fields = [f for f, _ in capi.QtosFeedback._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qtos_planner.h"\nint main(void) { printf("%d", (int)sizeof(QtosFeedback));\n'
                   + "".join('printf(" %%d", (int)offsetof(QtosFeedback, %s));\n' % f for f in fields)
                   + 'printf(" %d %d %d\\n", QTOS_FEEDBACK_QUAT, QTOS_FEEDBACK_SNAP, QTOS_FEEDBACK_ZERO_FILTER); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    assert got[0] == C.sizeof(capi.QtosFeedback) and got[1:-3] == [getattr(capi.QtosFeedback, f).offset for f in fields]
    assert got[-3:] == [capi.FEEDBACK_QUAT, capi.FEEDBACK_SNAP, capi.FEEDBACK_ZERO_FILTER] == [F.FLAG_QUAT, F.FLAG_SNAP, F.FLAG_ZERO_FILTER]
    cfg = PlannerConfig.reference_compat()
    p = capi.feedback_params(cfg)
    assert (p.gain_pos, p.gain_ang, p.gain_foot, p.max_pos, p.max_ang, p.max_foot, p.latency) == (1.0, 1.0, 1.0, 0.05, 0.2, 0.05, 0.0)
    assert p.flags == capi.FEEDBACK_SNAP and p.capacity == 0 and p.hz == 1000.0 and p.ee_shift == 0.015
    assert (p.rom_tol, p.snap_tol) == (1e-6, 0.02)
    assert [list(r) for r in p.nominal] == [list(r) for r in cfg.nominal_stance] and list(p.max_deviation) == list(cfg.max_deviation)
    assert [list(r) for r in p.hip] == J.SOLO12.hip.tolist() and p.l_upper == p.l_lower == 0.16
    q = capi.feedback_params(cfg, snap=False, zero_filter=True, quaternion=True, latency=0.02, gain_foot=0.25)
    assert q.flags == capi.FEEDBACK_QUAT | capi.FEEDBACK_ZERO_FILTER and q.latency == 0.02 and q.gain_foot == 0.25
    # the ctypes mirror is read by the rule as FeedbackParams is
    L, x = sp.layout(cfg), load_gv("gv1")["x"]
    r = 2000
    start = handover_start(L, x, r)
    meas = on_plan(L, x, r - 1, dtype=F64)
    meas[0:3] += D
    a = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas, F64), F.FeedbackParams(n_rows=r), start, dtype=F64)
    b = F.start_feedback(L, x, 0.0, r, table(r, r - 1, meas, F64), capi.feedback_params(cfg, n_rows=r), start, dtype=F64)
    assert a[3] == b[3] and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[2]), bits(b[2]))
