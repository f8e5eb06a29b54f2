"""The rollout kernel on the MI355X (pytest -m gpu): k_rollout against the longdouble statement of the rule (qtos_amd/rollout.py), its
exact columns, both forms of `meas`, table against ring, carried state, the tick, a non-default stream, the host form, the argument
checks, the call from plain C and the rollout of ShiftedWindows against the statement applied segment by segment.

Shapes.  TILE = 256 rows is the multi-wave tile.  A case is one plan (the golden walk, and the exp_5 step whose base pitches: two
planners) with B = 3 windows of it at 100 Hz, each with a clock of its own; n_rows = 2 TILE + 37, two full tiles and a partial one
with rows past the horizon (549 rows at 100 Hz are 5.48 s of a 5 s plan); the per-window counts are 0, exactly TILE and the full
count; window 2 has mass_scale 1.3 and a push.  The rate departs from the 200 Hz this test was specified with: the two other
conditions of that specification, n_rows = 2 TILE + 37 and rows past the horizon, cannot both hold there (549 rows at 200 Hz end at 2.74 s of the 5 s
plan), and they are the ones that select code paths -- the partial tile and the clamp of the plan time -- while the rate only
sets h; 200 Hz itself runs in tests/test_rollout_cpu.py, tests/c/rollout_caller.c runs 1 kHz and so does the ShiftedWindows
test below.  substeps 1 and 3.  Gains: "held", rollout_cases.GAINS with a force clip of 9.5 N
that acts on some of window 2's rows and not on all (asserted in the statement: its extra weight alone asks for 8.8 N), on the
physical inertia; and "free", no gains and ff_scale 0 --
with the plan's forces and no gains the body is an inverted pendulum (the torque -e x F grows with the drift: sqrt(m g z / I) is
about 34 / s), the float64 statement is O(1) off the longdouble one within a second, and by the rule of tests/rollout_cases.py such
a case is ill-conditioned and another is chosen: the free body, which still goes through every line of the step.

Accuracy gates (rollout_cases.gate: the larger of 8 x the float64-vs-longdouble floor of the numpy statement measured here and a
propagated bound, capped at 1e-10).  As tests/test_gpu_track.py states, no document with ROCm's ulp figures is installed next to the
compiler, so 4 ulp are ASSUMED for each of sin, cos, sqrt, atan2 and asin: 8 u relative, u = 2^-53.
  inputs   q_p is a sum of two products of three sines / cosines: 2 x (24 u + 3 u) = 54 u; w_p two products of two with a rate
           below 4 rad/s: 2 x 4 x (16 u + 2 u) = 144 u; F and tau_p take no library call
  state    the held body follows its inputs with a closed loop that is damped (kd / (2 sqrt(kp I)) > 1 on every axis): an input
           error comes out at most doubled, and the 3 sqrt of a step (8 u each on a unit quaternion, 549 x 3 steps, not
           accumulating in a damped loop beyond its memory of about 1 / (h kd / I) = 1 step) add 24 u: q, r within 2 x 54 u + 24 u,
           taken as POS = 256 u; the rates v, w_b and R w_b are stiffer by the loop's bandwidth sqrt(kp_ang / I_xx) = 72 / s and
           carry w_p's 144 u: 72 x 256 u + 2 x 144 u, taken as RATE = 2^15 u = 3.6e-12
  Euler    |pitch| <= 1.2: atan2 of two entries (each 4 POS off) at a radius >= 0.36 and 4 ulp of a result below pi: taken as
           EULER = 2^12 u
  |e|, tilt  sqrt of sums of POS-accurate differences: 2 POS + 8 u: taken as POS x 4
  |F_fb|   kp_lin x POS + kd_lin x RATE = 300 x 256 u + 30 x 2^15 u < 2^21 u = 2.3e-10 N: over the cap, which holds for this
           column as for every other, so the gate is 1e-10 N (measured: below 5e-13 N)
The free body has no loop: its r and v are the sums tests/test_rollout_cpu.py bounds (549 steps of 10 ms: |v| < 54 m/s, |r| < 150 m:
549 x 54 u < 2^15 u on v and 549 x (150 u + 0.01 x 2^15 u) < 2^18 u on r, 2.9e-11 m), and its rotation a product of 549 x 3
normalised steps, each 8 u + 16 u, 2^16 u: q is held to r's 2^18 u and R w_b to v's 2^15 u, the Euler angles and the norms to 2^19 u.
The time stamps, the joint columns, the counts and the status words are exact, but for bit 3 on rows where a feedback component
lies within the gate of its limit: those rows are found with the statement (limits scaled by 1 -+ 1e-9) and may be at most 1 % of
a window's rows; that the chosen gains and limit keep the statement within that, and that the clip acts, is checked without a GPU
in tests/test_rollout_cpu.py on the oracle's plans, and here once more on the plans the kernel gets.
Measured on an MI355X: profiles/rollout_accuracy.json."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_cases as rc
from conftest import ROOT, load_gv
from rollout_cases import (B, COUNT_IN, COUNTS, F64, HZ, LD, MASS_SCALE, N_ROWS, PUSH, PUSH_FROM, PUSH_TICKS, T0, TILE, U, body_kw)

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
STATE_IN = np.arange(B * 13, dtype=F64).reshape(B, 13) * 0.01 + 0.5        # (the INIT flag replaces it where a window has rows)
BOUNDS = {"held": dict(pos=256 * U, rate=2 ** 15 * U, euler=2 ** 12 * U, norm=1024 * U, fb=2 ** 21 * U),
          "free": dict(pos=2 ** 18 * U, rate=2 ** 15 * U, euler=2 ** 19 * U, norm=2 ** 19 * U, fb=0.0)}
GROUPS = dict(r=(slice(1, 4), "pos"), euler=(slice(4, 7), "euler"), v=(slice(7, 10), "rate"), Rw=(slice(10, 13), "rate"),
              q=(slice(13, 17), "pos"), norms=(slice(17, 19), "norm"), fb=(slice(19, 20), "fb"))
LLP = C.POINTER(C.c_longlong)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def gate_of(kind, key, floor):
    return rc.gate(floor, BOUNDS[kind][key])


class Case:
    """One plan: its planner, nodes, the joint table of B windows; kernel results and statements are made once per (kind, substeps)."""

    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name = name
        self.cfg = PlannerConfig.reference_compat()
        self.P = Planner(self.cfg, max_batch=8)
        if name == "walk":
            nodes = np.array(load_gv("gv1")["x"])[None]
        else:                                                   # a step onto the ledges of exp_5: the base pitches
            hxy, cell = workloads.exp5_terrain()
            self.P.set_heightfields(hxy, cell)
            start, goal = workloads.step_goals(1, seed=1, terrain=(hxy, cell))
            nodes, status, _, _ = self.P.plan(start, goal)
        self.nodes = np.repeat(nodes, B, axis=0)
        self.L = sp.layout(self.cfg)
        self.sample = self.P.sample(self.nodes, T0, hz=HZ, n_rows=N_ROWS)
        self.joint, _ = self.P.joint_rows(self.nodes, T0, capi.joint_params(hz=HZ, n_rows=N_ROWS, tau_max=0.0))
        self.joint.setflags(write=False)
        self._got, self._want = {}, {}

    def params(self, kind, sub, **kw):
        from qtos_amd import capi
        return capi.rollout_params(cfg=self.cfg, hz=HZ, n_rows=N_ROWS, init=True, **body_kw(kind, sub), **kw)

    def run(self, params, **kw):
        """The base call: per-window counts, a state, count and word that stand, meas / rows / status pre-filled."""
        mcols = 19 if params.flags & 2 else 18
        args = dict(n_rows=COUNTS, joint=self.joint, mass_scale=MASS_SCALE, push=PUSH, state=STATE_IN, count=COUNT_IN, word=np.zeros(B, np.int32),
                    meas=np.full((B, N_ROWS, mcols), -7.5), rows=np.full((B, N_ROWS, 20), -7.5), status=np.full((B, N_ROWS), -7, np.int32))
        args.update(kw)
        return self.P.rollout(self.nodes, T0, params, **args)

    def got(self, kind, sub):
        if (kind, sub) not in self._got:
            self._got[kind, sub] = self.run(self.params(kind, sub))
        return self._got[kind, sub]

    def statement(self, kind, sub, b, dt, n=None, scale=1.0):
        return rc.window_statement(self.L, self.cfg, self.nodes[b], kind, sub, b, dt, n=n, scale=scale, joint=self.joint[b])

    def want(self, kind, sub):
        if (kind, sub) not in self._want:
            self._want[kind, sub] = {dt: [self.statement(kind, sub, b, dt) for b in range(B)] for dt in (F64, LD)}
        return self._want[kind, sub]


_cases = {}


@pytest.fixture(params=["walk", "exp5"])
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


@pytest.mark.parametrize("sub", [1, 3])
@pytest.mark.parametrize("kind", ["held", "free"])
def test_kernel_against_the_statement(case, kind, sub):
    from qtos_amd import rollout as ro
    meas, rows, status, state, count, word = case.got(kind, sub)
    want = case.want(kind, sub)
    assert N_ROWS > 2 * TILE and (N_ROWS - 1) / HZ > case.L.T                           # a partial third tile, rows past the horizon
    assert np.array_equal(bits(state[0]), bits(STATE_IN[0])) and count[0] == COUNT_IN[0] and word[0] == 0     # no rows: kept
    assert count[1:].tolist() == [TILE, 2 + N_ROWS]
    entry = {}
    for b in (1, 2):
        n = int(COUNTS[b])
        w64, wld = want[F64][b], want[LD][b]
        assert (meas[b, n:] == -7.5).all() and (rows[b, n:] == -7.5).all() and (status[b, n:] == -7).all()    # untouched behind the count
        assert np.array_equal(bits(rows[b, :n, 0]), bits(case.sample[b, :n, 0]))                               # qtos_sample_csv's stamps
        assert np.array_equal(bits(meas[b, :n, 6:18]), bits(case.joint[b, :n, 1:13]))                          # the joint table's angles
        assert np.array_equal(bits(meas[b, :n, 0:6]), bits(rows[b, :n, 1:7]))
        assert float(np.abs(wld[1][:, 5]).max()) <= 1.2 and not (wld[2] & (ro.FALLEN | ro.NONFINITE | ro.GIMBAL)).any()       # (the Euler bound's pitch)
        e = {}
        for name, (cols, key) in GROUPS.items():
            floor = rc.dist(w64[1][:, cols], wld[1][:, cols])
            e[name] = dict(floor=floor, gate=gate_of(kind, key, floor), error=rc.dist(rows[b, :n, cols], wld[1][:, cols]))
        floor = rc.dist(w64[3], wld[3])
        e["state"] = dict(floor=floor, gate=max(gate_of(kind, "rate", floor), gate_of(kind, "pos", floor)), error=rc.dist(state[b], wld[3]))
        entry["window%d" % b] = e
        # the status words: exact, but for bit 3 where a component lies within the gate of its limit
        near = np.zeros(n, bool)
        if kind == "held":
            clipped = (wld[2] & ro.CLIPPED) != 0
            assert clipped.sum() < n and (b == 1 or clipped.sum() > 0), clipped.sum()  # the clip acts on window 2, and not everywhere
            near = rc.near_the_limit(*(case.statement(kind, sub, b, LD, scale=s)[2] for s in (1 - rc.NEAR, 1 + rc.NEAR)))
            assert near.sum() <= n // 100, np.nonzero(near)[0]
            e["rows_near_the_limit"] = np.nonzero(near)[0].tolist()
        mask = np.where(near, ~np.int32(ro.CLIPPED), ~np.int32(0))
        assert np.array_equal(status[b, :n] & mask, wld[2] & mask) and word[b] == wld[5] == 0
        j = np.arange(n)
        acts = (COUNT_IN[b] + j >= PUSH_FROM) & (COUNT_IN[b] + j < PUSH_FROM + PUSH_TICKS)
        assert np.array_equal((status[b, :n] & ro.PUSH) != 0, acts) and acts.sum() == (PUSH_TICKS if b == 2 else 0)
    rc.record("gpu_%s_%s_substeps%d" % (case.name, kind, sub), entry)
    for e in entry.values():
        for name, v in e.items():
            if isinstance(v, dict):
                assert v["error"] <= v["gate"], (case.name, kind, sub, name, v)


def test_quaternion_form_of_meas(case):
    meas, rows, status, state, count, word = case.got("held", 1)
    q = case.run(case.params("held", 1, quaternion=True))
    assert q[0].shape == (B, N_ROWS, 19)
    for b in (1, 2):
        n = int(COUNTS[b])
        assert np.array_equal(bits(q[0][b, :n, 0:3]), bits(rows[b, :n, 1:4])) and np.array_equal(bits(q[0][b, :n, 3:7]), bits(rows[b, :n, 13:17]))
        assert np.array_equal(bits(q[0][b, :n, 7:19]), bits(case.joint[b, :n, 1:13])) and (q[0][b, n:] == -7.5).all()
    assert np.array_equal(bits(q[1]), bits(rows)) and np.array_equal(q[2], status) and np.array_equal(bits(q[3]), bits(state))
    # without a joint table the twelve columns are left as they are
    bare = case.run(case.params("held", 1), joint=None)
    assert (bare[0][2, :, 6:18] == -7.5).all() and np.array_equal(bits(bare[0][2, :, 0:6]), bits(meas[2, :, 0:6]))
    none = case.run(case.params("held", 1), rows=None)
    assert none[1] is None and np.array_equal(bits(none[0]), bits(meas)) and np.array_equal(none[2], status)


def one_window(case, b, params, **kw):
    args = dict(joint=case.joint[b:b + 1, :params.n_rows] if params.capacity == 0 else None, mass_scale=MASS_SCALE[b:b + 1], push=PUSH[b:b + 1],
                count=COUNT_IN[b:b + 1])
    args.update(kw)
    return case.P.rollout(case.nodes[b:b + 1], T0[b:b + 1], params, **args)


def test_two_segments_with_the_carried_state_are_one_call(case):
    from qtos_amd import capi
    b, cut = 2, 300
    meas, rows, status, state, count, word = case.got("held", 3)
    kw = body_kw("held", 3)
    first = one_window(case, b, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=cut, init=True, **kw))
    p2 = capi.rollout_params(cfg=case.cfg, hz=HZ, first_row=cut, n_rows=N_ROWS - cut, **kw)
    second = one_window(case, b, p2, joint=case.joint[b:b + 1, cut:], state=first[3], count=first[4], word=first[5])
    assert np.array_equal(bits(np.concatenate([first[0], second[0]], 1)), bits(meas[b:b + 1]))
    assert np.array_equal(bits(np.concatenate([first[1], second[1]], 1)), bits(rows[b:b + 1]))
    assert np.array_equal(np.concatenate([first[2], second[2]], 1), status[b:b + 1])
    assert np.array_equal(bits(second[3][0]), bits(state[b])) and second[4][0] == count[b] and second[5][0] == word[b]


def test_a_pending_word_sets_each_window_on_its_plan_at_its_first_rows(case):
    """No INIT flag, QTOS_ROLLOUT_PENDING in every window's word: window 0 (no rows) keeps its state, its count and the bit, windows
    1 and 2 give the INIT call's rows to the bit and clear it.  A second call that gives rows to window 0 alone sets it on its plan
    then (the rows of an INIT call of its own), and leaves the others as they are."""
    from qtos_amd import capi
    meas, rows, status, state, count, word = case.got("held", 3)
    kw = body_kw("held", 3)
    p = capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=N_ROWS, **kw)
    assert not p.flags & capi.ROLLOUT_INIT
    got = case.run(p, word=np.full(B, capi.ROLLOUT_PENDING, np.int32))
    assert np.array_equal(bits(got[0]), bits(meas)) and np.array_equal(bits(got[1]), bits(rows)) and np.array_equal(got[2], status)
    assert np.array_equal(bits(got[3]), bits(state)) and np.array_equal(got[4], count)
    assert got[5].tolist() == [capi.ROLLOUT_PENDING, 0, 0]
    assert not any((got[2][b, :COUNTS[b]] & capi.ROLLOUT_PENDING).any() for b in (1, 2))          # (never a row's status)
    second = case.run(p, n_rows=np.array([TILE, 0, 0], np.int32), state=got[3], count=got[4], word=got[5])
    own = one_window(case, 0, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=TILE, init=True, **kw))
    assert np.array_equal(bits(second[1][0, :TILE]), bits(own[1][0])) and np.array_equal(bits(second[0][0, :TILE]), bits(own[0][0]))
    assert np.array_equal(second[2][0, :TILE], own[2][0]) and np.array_equal(bits(second[3][0]), bits(own[3][0]))
    assert second[5].tolist() == [0, 0, 0] and second[4].tolist() == [COUNT_IN[0] + TILE, count[1], count[2]]
    assert np.array_equal(bits(second[3][1:]), bits(state[1:])) and (second[1][1:] == -7.5).all()


def test_ring_mode_is_the_table(case):
    """Capacity 300, two appends of 200 rows from cursor 130: the first wraps inside its first tile, the second lies over the first's
    oldest rows.  The rings' rows are the table-mode rows of the same row numbers, to the bit."""
    from qtos_amd import capi
    from qtos_amd.stitcher import ring_rows
    cap, seg, b, cur0 = 300, 200, 2, 130
    kw = body_kw("held", 1)
    table = one_window(case, b, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=2 * seg, init=True, **kw))
    ring_m, ring_r, ring_s = np.full((1, cap, 18), -7.5), np.full((1, cap, 20), -7.5), np.full((1, cap), -7, np.int32)
    ring_j = np.full((1, cap, 37), np.nan)
    cursor, state, count, word = cur0, None, COUNT_IN[b:b + 1], None
    for i in range(2):
        at = (cursor + np.arange(seg)) % cap
        ring_j[0, at] = case.joint[b, i * seg:(i + 1) * seg]
        p = capi.rollout_params(cfg=case.cfg, hz=HZ, first_row=i * seg, n_rows=seg, capacity=cap, init=i == 0, **kw)
        ring_m, ring_r, ring_s, state, count, word = one_window(case, b, p, joint=ring_j, cursor=np.array([cursor], np.int64), state=state,
                                                                count=count, word=word, meas=ring_m, rows=ring_r, status=ring_s)
        if i == 0:
            free = np.setdiff1d(np.arange(cap), at)
            assert (ring_r[0, free] == -7.5).all() and (ring_s[0, free] == -7).all() and (ring_m[0, free] == -7.5).all()
        cursor += seg
    for ring, tab in ((ring_m, table[0]), (ring_r, table[1])):
        assert np.array_equal(bits(ring_rows(ring[0], cursor)), bits(tab[0, -cap:]))
    assert np.array_equal(ring_rows(ring_s[0], cursor), table[2][0, -cap:])
    assert np.array_equal(bits(state), bits(table[3])) and count[0] == table[4][0] and word[0] == table[5][0]


def test_tick_of_five_robots(case):
    """B = 5, one row each at a row index of its own, from the state the table's kernel carries there: the one-wave instantiation's
    rows are the table's rows, to the bit."""
    from qtos_amd import capi
    n, b = 5, 2
    first = np.array([1, 2, TILE - 1, TILE, N_ROWS - 1], np.int32)
    meas, rows, status, state, count, word = case.got("held", 3)
    kw = body_kw("held", 3)
    nodes, t0 = np.repeat(case.nodes[b:b + 1], n, axis=0), np.repeat(T0[b:b + 1], n)
    shared = dict(mass_scale=np.repeat(MASS_SCALE[b], n), push=np.repeat(PUSH[b:b + 1], n, axis=0))
    upto = case.P.rollout(nodes, t0, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=N_ROWS, init=True, **kw), n_rows=first,
                          joint=np.repeat(case.joint[b:b + 1], n, axis=0), count=np.repeat(COUNT_IN[b], n), **shared)
    assert upto[4].tolist() == (COUNT_IN[b] + first).tolist()
    tick = case.P.rollout(nodes, t0, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=1, **kw), first_row=first,
                          joint=case.joint[b, first][:, None, :], state=upto[3], count=upto[4], word=upto[5], **shared)
    assert tick[1].shape == (n, 1, 20)
    assert np.array_equal(bits(tick[1][:, 0]), bits(rows[b, first])) and np.array_equal(bits(tick[0][:, 0]), bits(meas[b, first]))
    assert np.array_equal(tick[2][:, 0], status[b, first]) and tick[4].tolist() == (COUNT_IN[b] + first + 1).tolist()
    assert np.array_equal(bits(tick[3][-1]), bits(state[b]))                              # behind the last row: the table's carried state
    # a full wave of the one-wave kernel, and one row more (the 256-lane kernel): the table's rows, to the bit
    pre = one_window(case, b, capi.rollout_params(cfg=case.cfg, hz=HZ, n_rows=100, init=True, **kw))
    for m in (64, 65):
        part = one_window(case, b, capi.rollout_params(cfg=case.cfg, hz=HZ, first_row=100, n_rows=m, **kw), joint=case.joint[b:b + 1, 100:100 + m],
                          state=pre[3], count=pre[4], word=pre[5])
        assert np.array_equal(bits(part[1][0]), bits(rows[b, 100:100 + m])) and np.array_equal(bits(part[0][0]), bits(meas[b, 100:100 + m]))
        assert np.array_equal(part[2][0], status[b, 100:100 + m])


def test_device_form_on_a_held_up_stream_is_the_host_form(case):
    import torch
    dev = torch.device("cuda", 0)
    meas, rows, status, state, count, word = case.got("held", 3)
    p = case.params("held", 3)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0, d_n = torch.as_tensor(T0, **f64), torch.as_tensor(COUNTS, device=dev)
    d_joint, d_ms, d_push = torch.as_tensor(np.array(case.joint), **f64), torch.as_tensor(MASS_SCALE, **f64), torch.as_tensor(PUSH, **f64)
    src = torch.as_tensor(case.nodes, **f64)
    side = torch.cuda.Stream(dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)              # (elementwise work: holds the stream up, loads no BLAS library)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        o_m, o_r = torch.full((B, N_ROWS, 18), -7.5, **f64), torch.full((B, N_ROWS, 20), -7.5, **f64)
        o_s = torch.full((B, N_ROWS), -7, dtype=torch.int32, device=dev)
        d_state, d_count, d_word = torch.as_tensor(STATE_IN, **f64), torch.as_tensor(COUNT_IN, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if stream is side:
                for _ in range(50):
                    busy.mul_(1.0001).clamp_(0.0, 1.0)
            d_nodes = src + 0.0
            r = case.P.lib.qtos_rollout_device(case.P.h, B, C.byref(p), d_nodes.data_ptr(), d_t0.data_ptr(), None, d_n.data_ptr(), None,
                                               d_joint.data_ptr(), d_ms.data_ptr(), d_push.data_ptr(), d_state.data_ptr(), d_count.data_ptr(),
                                               d_word.data_ptr(), o_m.data_ptr(), o_r.data_ptr(), o_s.data_ptr(), C.c_void_p(stream.cuda_stream))
            assert r == 0, case.P.lib.qtos_last_error(case.P.h)
        stream.synchronize()
        assert np.array_equal(bits(o_m.cpu().numpy()), bits(meas)) and np.array_equal(bits(o_r.cpu().numpy()), bits(rows))
        assert np.array_equal(o_s.cpu().numpy(), status) and np.array_equal(bits(d_state.cpu().numpy()), bits(state))
        assert np.array_equal(d_count.cpu().numpy(), count) and np.array_equal(d_word.cpu().numpy(), word)
    torch.cuda.synchronize()


def test_argument_checks(case):
    from qtos_amd import capi
    cap = 300
    p = capi.rollout_params(cfg=case.cfg, hz=HZ, first_row=40, n_rows=200, capacity=cap, **body_kw("held", 1))
    meas, rows, st = np.zeros((1, cap, 18)), np.zeros((1, cap, 20)), np.zeros((1, cap), np.int32)
    state, count, word = np.zeros((1, 13)), np.zeros(1, np.int64), np.zeros(1, np.int32)
    state[0, 9] = 1.0

    def call(**kw):
        a = dict(h=case.P.h, b=1, s=p, nodes=case.nodes[:1], t0=T0[:1], cur=np.array([0], np.int64), state=state.copy(), count=count.copy(),
                 word=word.copy(), meas=meas.copy(), rows=rows.copy(), st=st.copy())
        a.update(kw)
        ll = lambda v: None if v is None else v.ctypes.data_as(LLP)
        return case.P.lib.qtos_rollout(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]), None,
                                       None, ll(a["cur"]), None, None, None, capi._dp(a["state"]), ll(a["count"]), capi._ip(a["word"]),
                                       capi._dp(a["meas"]), capi._dp(a["rows"]), capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            if key == "inertia_b":
                for i in range(9):
                    s.inertia_b[i] = v[i]
            else:
                setattr(s, key, v)
        return s
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null t0": call(t0=None), "null state": call(state=None), "null count": call(count=None), "null word": call(word=None),
           "null meas": call(meas=None), "null status": call(st=None), "ring without cursor": call(cur=None),
           "capacity < 0": call(s=params(capacity=-1)), "table without rows": call(s=params(capacity=0, n_rows=0)),
           "first_row -1": call(s=params(first_row=-1)), "first_row 1000001": call(s=params(first_row=1000001)),
           "n_rows < 0": call(s=params(n_rows=-1)), "substeps 0": call(s=params(substeps=0)), "hz 0": call(s=params(hz=0.0)),
           "hz nan": call(s=params(hz=float("nan"))), "mass 0": call(s=params(mass=0.0)), "push_ticks < 0": call(s=params(push_ticks=-1)),
           "singular inertia": call(s=params(inertia_b=[1.0, 2.0, 3.0, 2.0, 4.0, 6.0, 0.0, 0.0, 1.0]))}
    assert all(v == -1 for v in got.values()), got
    assert b"inertia_b is singular" in case.P.lib.qtos_last_error(case.P.h)
    call(s=params(substeps=0))
    assert b"substeps" in case.P.lib.qtos_last_error(case.P.h)
    assert call() == 0 and call(s=params(first_row=1000000)) == 0 and call(rows=None) == 0


def test_rollout_from_plain_c(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "rollout_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "rollout_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_rollout=%d rollout_null=-1 rollout_device_null=-1" % C.sizeof(capi.QtosRollout)
    assert lines[1].startswith("bad_args=" + ",".join(["-1"] * 8) + " reason=qtos_rollout: first_row")
    assert lines[2] == "plan rc=0 status=0,0"
    kv = dict(t.split("=") for t in lines[3].replace("rollout rc", "rollout_rc").split())
    assert int(kv["rollout_rc"]) == 0 and int(kv["mismatches"]) == 0 and kv["word"] == "0,0"
    assert 0 < float(kv["worst_e"]) < 0.02                       # a trot's forces between its knots, held by the gains
    kv = dict(t.split("=") for t in lines[4].replace("track rc", "track_rc").split())
    assert int(kv["track_rc"]) == 0 and float(kv["worst_foot"]) < 0.05 and kv["recorded"] == "799,799"       # (delay 0 of the reference rule: call 1 is skipped)


def test_rollout_of_shifted_windows_is_the_statement_segment_by_segment():
    """B = 4, three replans of 420 rows into rings of 1000 (the third append wraps), joints, track, feedback and the rollout on,
    window 3 pushed: behind every replan the measured ring's rows of the segment are the statement's, applied segment by segment
    with the state, count and word it carries itself in longdouble, at the held body's gates; the status words are the statement's but for bit 3 on rows near the limit (found as the
    kernel test finds them, at most 1 % of a segment; the 7 N clip acts: the push alone asks for 6.7 N); k_track's rows of that ring are
    k_track's rows of the statement's ring (the pose within the rollout's gates carried through the leg: 4 x POS + EULER on a foot
    0.45 m from the CoM, its errors likewise, the totals that times the recorded rows); the pushed window's start is corrected.
    Sets without the new keyword allocate nothing of the rollout and queue nothing (their _rollout_rows is replaced by a function
    that raises), and two of them give the same plans, rings, cursors and clocks.  That comparison is between two runs of this code:
    it shows that the plain path is deterministic and never reaches the rollout, not by itself that its bits are those of the code
    before the keyword existed -- what holds that is that the plain path's rings and hand-overs keep passing the tests they
    had (tests/test_gpu_stitch.py, test_gpu_handover.py, test_gpu_feedback.py), which compare them with their own rules."""
    import torch
    from oracle import splines as sp
    from qtos_amd import capi, rollout as ro, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import INERTIA_PHYSICAL, PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    nb, cap, seg = 4, 1000, 420
    cfg = PlannerConfig.knots100(gait="trot")
    L = sp.layout(cfg)
    start, goal = workloads.flat_goals(nb, seed=7)
    P = Planner(cfg, max_batch=nb)
    host = lambda t: t.cpu().numpy().copy()
    push = np.zeros((nb, 6))
    push[3] = (6.0, 3.0, 0.0, 0.0, 0.0, 0.05)
    body = dict(inertia_b=INERTIA_PHYSICAL, substeps=2, f_fb_max=7.0, push_from=500, push_ticks=200, dev_max=0.5, tilt_max=1.0, **rc.GAINS)
    scale = np.array([1.0, 1.1, 1.0, 1.0])
    try:
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, rollout=dict(cfg=cfg))
        plain = []
        for _ in range(2):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, stream=torch.cuda.Stream())
            assert W._rollout is None and not hasattr(W, "rollout_state") and not hasattr(W, "rollout_status") and not hasattr(W, "meas_traj")

            def never(*a):
                raise AssertionError("a rollout was queued")
            W._rollout_rows = never
            with pytest.raises(RuntimeError):
                W.rollout_rows(0)
            for _ in range(4):
                W.replan()
            W.finish()
            torch.cuda.synchronize()
            plain.append([host(W.nodes), host(W.traj), host(W.cursor), host(W.t0)])
        for a, b in zip(*plain):
            assert a.tobytes() == b.tobytes()
        W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(tau_max=3.0),
                           track=dict(delay=0, rule="clean"), feedback=dict(cfg=cfg), stream=torch.cuda.Stream(),
                           rollout=dict(cfg=cfg, mass_scale=scale, push=push, rows=True, **body))
        W.replan()
        torch.cuda.synchronize()
        assert (host(W.rollout_word) == capi.ROLLOUT_PENDING).all() and (host(W.rollout_count) == 0).all()    # no plan to hand over from yet
        rp = ro.RolloutParams(cfg, **body)
        side = [ro.RolloutParams(cfg, **dict(body, f_fb_max=body["f_fb_max"] * s)) for s in (1 - rc.NEAR, 1 + rc.NEAR)]
        carried = [dict(state=None, count=0, word=ro.PENDING) for _ in range(nb)]
        beside = [[dict(state=None, count=0, word=ro.PENDING) for _ in range(nb)] for _ in side]
        count = total = None
        entry = {}
        for i in range(3):
            h_nodes, h_t0, cur = host(W.nodes), host(W.t0), host(W.cursor)
            W.replan()
            torch.cuda.synchronize()
            assert (host(W.row) == seg).all() and (host(W.cursor) == cur + seg).all()
            at = (cur[0] + np.arange(seg)) % cap
            meas, rows, st = host(W.meas_traj)[:, at], host(W.rollout_traj)[:, at], host(W.rollout_status)[:, at]
            joint, _ = P.joint_rows(h_nodes, h_t0, capi.joint_params(hz=1000.0, n_rows=seg, tau_max=3.0))
            want = np.zeros((nb, seg, 18))
            for b in range(nb):
                c = carried[b]
                m, r, s, c["state"], c["count"], c["word"] = ro.rollout_rows(L, h_nodes[b], h_t0[b], 1000.0, 0, seg, rp, state=c["state"], count=c["count"],
                                                                           word=c["word"], mass_scale=scale[b], push=push[b], joint=joint[b], dtype=LD)
                want[b] = m.astype(F64)
                lohi = []
                for sp_, cs in zip(side, beside):                                  # the limit a little lower and a little higher, each carried by itself
                    o = ro.rollout_rows(L, h_nodes[b], h_t0[b], 1000.0, 0, seg, sp_, mass_scale=scale[b], push=push[b], dtype=LD, **cs[b])
                    cs[b].update(state=o[3], count=o[4], word=o[5])
                    lohi.append(o[2])
                near = rc.near_the_limit(*lohi)
                assert near.sum() <= seg // 100, (i, b, np.nonzero(near)[0])
                mask = np.where(near, ~np.int32(ro.CLIPPED), ~np.int32(0))
                e = dict(clipped=int(((s & ro.CLIPPED) != 0).sum()), near=np.nonzero(near)[0].tolist(), pos=rc.dist(meas[b, :, 0:3], m[:, 0:3]), euler=rc.dist(meas[b, :, 3:6], m[:, 3:6]), rate=rc.dist(rows[b, :, 7:13], r[:, 7:13]))
                entry["replan%d_window%d" % (i, b)] = e
                assert e["pos"] <= BOUNDS["held"]["pos"] * 4 and e["euler"] <= BOUNDS["held"]["euler"] and e["rate"] <= BOUNDS["held"]["rate"], (i, b, e)
                assert np.array_equal(bits(meas[b, :, 6:18]), bits(joint[b, :, 1:13])) and np.array_equal(st[b] & mask, s & mask)
                assert ((st[b] & ro.PUSH) != 0).sum() == len(np.intersect1d(np.arange(i * seg, (i + 1) * seg), np.arange(500, 700)))
            assert host(W.rollout_count).tolist() == [(i + 1) * seg] * nb and (host(W.rollout_word) == 0).all()
            # k_track on the kernel's ring against k_track on the statement's ring
            tr = host(W.track_traj)[:, at]
            tab = P.track(h_nodes, h_t0, want, capi.track_params(hz=1000.0, n_rows=seg, delay=0, rule="clean"), count=count, total=total)
            count, total = tab[2], tab[3]
            tol = 4 * (4 * BOUNDS["held"]["pos"] + BOUNDS["held"]["euler"])
            assert np.abs(tr[:, :, 1:24] - tab[0][:, :, 1:24]).max() <= tol and np.array_equal(bits(tr[:, :, 0]), bits(tab[0][:, :, 0]))
            assert np.abs(host(W.track_total) - total).max() <= 4 * tol * (i + 1) * seg and np.array_equal(host(W.track_count), count)
            fb = host(W.feedback_status)
            if i >= 1:
                assert fb[3] & 1, fb                                                   # the pushed window's start moved to where its body is
        assert float(np.abs(host(W.meas_traj)[3, :, 0:3] - host(W.traj)[3, :, 1:4]).max()) > 1e-3          # the push is seen
        W.finish()
        torch.cuda.synchronize()
        assert host(W.rollout_count).tolist() == [3 * seg + 5001] * nb
        r3, s3 = W.rollout_rows(3)
        assert r3.shape == (cap, 20) and s3.shape == (cap,) and np.array_equal(bits(r3[:, 0]), bits(W.trajectory_rows(3)[:, 0]))
        assert sum(e["clipped"] for e in entry.values()) > 0                           # the 7 N clip acted: bit 3 was compared where it is set
        rc.record("gpu_shifted_windows", entry)
    finally:
        P.close()
