"""The kernel of the rollout through the feet on the MI355X (pytest -m gpu): k_rollout_feet against the longdouble rule
(qtos_amd/rollout_feet.py), its exact columns, table against ring, carried state, the tick, a held-up side stream against the host
form, r and v against qtos_rollout's own output without gains, the argument checks, the call from plain C and the feet switch of
ShiftedWindows against the rule applied segment by segment.

Shapes: tests/rollout_cases.py's, the ones at which k_rollout can go wrong -- B = 3 windows of one plan at 100 Hz (the trot: 101 Hz,
below) x 549 rows (two full 256-row tiles and a partial one, rows past the 5 s horizon), counts 0 / 256 / 549, window 2 1.3 x as heavy and pushed,
substeps 1 and 3.  Plans: the golden walk (three and four stance feet, 24 rows of window 2 with two) and the device's trot of
tests/test_gpu_force_fit.py (two stance feet on most rows, four on the others; the gait has no flight rows -- rows without a stance
foot are in tests/test_rollout_feet_cpu.py).  Gains: rollout_cases.GAINS with a force clip of 20 N (it acts on some rows of the
heavy window), dev_max 0.15 m, tilt_max 0.3 rad -- tight, so that a body on its way down is frozen before its fall has amplified the
roundings: the heavy pushed trot cannot be held by two feet and falls in both settings, and its rows run through the freeze.  Two settings of the feet:
  free     damping 1e-6 (the default), no limit
  limited  QTOS_FEET_LIMIT with mu 0.7 and f_max 30 N, damping 1e-2
The limited setting has the larger damping for a reason: a row may not lie within the gate of a limit's threshold, the gate of a
force is K e~ with K the condition number of M (tests/rollout_feet_cases.py), and a stance force starts and ends at 0 N, the
threshold of "no pulling": with damping 1e-6 K is 5e6 on two-stance rows and the gate 1e-3 N, which some row of a 5 s plan always
comes nearer to than that; with damping 1e-2 K is below 1e3 and the gate below 3e-7 N.

The trot runs at 101 Hz: its phase switches are the multiples of 0.3125 s, and at 100 Hz the rows 125, 250 and 375 lie ON a switch,
where every foot's planned force is zero but for roundings and the load weights are ratios of those roundings -- any two
evaluations of such a row differ by what the feedback asks for, not by roundings.  At 101 Hz no row of the 549 lies on a switch but
those at the horizon's end, where all feet stand.  The case is changed, not the share of rows compared.

Gates: tests/rollout_feet_cases.py -- per column group the larger of 8 x the float64 numpy floor measured here on the same rows
and the propagated bound, amplified by the measured condition number of M (the feet columns per stance count, each with its own
K).  The time stamps, the joint columns, the counts and the status words are exact, on every row: the rule reports per row how near
a compared value -- of a feedback clip, of the limit -- came to its threshold in any step of the tick, and the test asserts that
this is further than the row's gate (K of the row's own M, and 8 x the float64 floor of the row's own forces), and that |e| and the tilt of a row are further from dev_max and
tilt_max than theirs.  The share of rows left out is 0.  Measured on an MI355X: profiles/rollout_feet_accuracy.json."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rollout_feet_cases as fc
from conftest import ROOT, load_gv
from rollout_cases import B, COUNT_IN, COUNTS, F64, LD, MASS_SCALE, N_ROWS, PUSH, PUSH_FROM, PUSH_TICKS, T0, TILE

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
STATE_IN = np.arange(B * 13, dtype=F64).reshape(B, 13) * 0.01 + 0.5        # (the INIT flag replaces it where a window has rows)
FEET = {"free": dict(), "limited": dict(limit=True, mu=0.7, f_max=30.0, damping=1e-2)}
LLP = C.POINTER(C.c_longlong)
DEV_MAX, TILT_MAX = 0.15, 0.3


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def body_kw(sub, **kw):
    from qtos_amd.config import INERTIA_PHYSICAL
    return dict(inertia_b=INERTIA_PHYSICAL, substeps=sub, push_from=PUSH_FROM, push_ticks=PUSH_TICKS, f_fb_max=20.0, dev_max=DEV_MAX, tilt_max=TILT_MAX,
                **dict(fc.GAINS, **kw))


class Case:
    """One plan: its planner, nodes, the joint table of B windows; kernel results and rules are made once per (feet, substeps)."""

    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name = name
        self.hz = 100.0 if name == "walk" else 101.0                # (the module's docstring: the trot's switches lie on the 100 Hz grid)
        self.cfg = PlannerConfig.reference_compat() if name == "walk" else PlannerConfig.reference_compat(gait="trot")
        self.P = Planner(self.cfg, max_batch=8)
        if name == "walk":
            nodes = np.array(load_gv("gv1")["x"])[None]
        else:
            start = workloads.rest_start(0.1)[None]
            nodes, status, _, _ = self.P.plan(start, np.array([[0.1 + 0.09 * self.cfg.duration, 0.0, 0.24]]))
            assert status[0] == 0
        self.nodes = np.repeat(nodes, B, axis=0)
        self.L = sp.layout(self.cfg)
        self.sample = self.P.sample(self.nodes, T0, hz=self.hz, n_rows=N_ROWS)
        self.joint, _ = self.P.joint_rows(self.nodes, T0, capi.joint_params(hz=self.hz, n_rows=N_ROWS, tau_max=0.0))
        self.joint.setflags(write=False)
        self._got, self._want = {}, {}

    def params(self, feet, sub, body=None, **kw):
        from qtos_amd import capi
        args = dict(cfg=self.cfg, hz=self.hz, n_rows=N_ROWS, init=True)
        args.update(kw)
        return capi.rollout_feet_params(**args, **FEET[feet], **(body_kw(sub) if body is None else body))

    def run(self, params, **kw):
        """The base call: per-window counts, a state, count and word that stand, meas / rows / frows / status pre-filled."""
        mcols = 19 if params.flags & 2 else 18
        args = dict(n_rows=COUNTS, joint=self.joint, mass_scale=MASS_SCALE, push=PUSH, state=STATE_IN, count=COUNT_IN, word=np.zeros(B, np.int32),
                    meas=np.full((B, N_ROWS, mcols), -7.5), rows=np.full((B, N_ROWS, 20), -7.5), frows=np.full((B, N_ROWS, 16), -7.5),
                    status=np.full((B, N_ROWS), -7, np.int32))
        args.update(kw)
        return self.P.rollout_feet(self.nodes, T0, params, **args)

    def got(self, feet, sub):
        if (feet, sub) not in self._got:
            self._got[feet, sub] = self.run(self.params(feet, sub))
        return self._got[feet, sub]

    def rule(self, feet, sub, b, dt):
        from qtos_amd import rollout as ro, rollout_feet as rf
        return rf.rollout_feet_rows(self.L, self.nodes[b], T0[b], self.hz, 0, int(COUNTS[b]), ro.RolloutParams(self.cfg, **body_kw(sub)),
                                    rf.FeetParams(self.cfg, **FEET[feet]), count=int(COUNT_IN[b]), mass_scale=MASS_SCALE[b], push=PUSH[b],
                                    joint=self.joint[b], dtype=dt, detail=True)

    def want(self, feet, sub):
        if (feet, sub) not in self._want:
            self._want[feet, sub] = {dt: [None if b == 0 else self.rule(feet, sub, b, dt) for b in range(B)] for dt in (F64, LD)}
        return self._want[feet, sub]


_cases = {}


@pytest.fixture(params=["walk", "trot"])
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


def row_conditions(M):
    M = np.asarray(M, F64)
    return np.array([float(np.linalg.cond(m)) if np.abs(m).max() > 0 else 1.0 for m in M])


@pytest.mark.parametrize("sub", [1, 3])
@pytest.mark.parametrize("feet", ["free", "limited"])
def test_kernel_against_the_rule(case, feet, sub):
    from qtos_amd import rollout as ro, rollout_feet as rf
    meas, rows, frows, status, state, count, word = case.got(feet, sub)
    want = case.want(feet, sub)
    assert N_ROWS > 2 * TILE and (N_ROWS - 1) / case.hz > case.L.T                           # a partial third tile, rows past the horizon
    assert np.array_equal(bits(state[0]), bits(STATE_IN[0])) and count[0] == COUNT_IN[0] and word[0] == 0     # no rows: kept
    assert (frows[0] == -7.5).all() and (rows[0] == -7.5).all() and count[1:].tolist() == [TILE, 2 + N_ROWS]
    entry = {}
    for b in (1, 2):
        n = int(COUNTS[b])
        w64, wld = want[F64][b], want[LD][b]
        det = wld[7]
        assert (meas[b, n:] == -7.5).all() and (rows[b, n:] == -7.5).all() and (frows[b, n:] == -7.5).all() and (status[b, n:] == -7).all()
        assert np.array_equal(bits(rows[b, :n, 0]), bits(case.sample[b, :n, 0])) and np.array_equal(bits(frows[b, :n, 0]), bits(rows[b, :n, 0]))
        assert np.array_equal(bits(meas[b, :n, 6:18]), bits(case.joint[b, :n, 1:13]))                          # the joint table's angles
        assert np.array_equal(bits(meas[b, :n, 0:6]), bits(rows[b, :n, 1:7]))
        st_ld = wld[3]
        assert float(np.abs(np.asarray(wld[1][:, 5], F64)).max()) <= 1.2 and not (st_ld & (ro.NONFINITE | ro.GIMBAL)).any()
        alive = (st_ld & (ro.FALLEN | ro.NONFINITE)) == 0
        Krow = row_conditions(w64[7]["M"])
        K = float(Krow[alive].max())
        cnt = det["stance"].sum(axis=1)
        e = dict(cond=K, stance_counts=np.bincount(cnt, minlength=5).tolist(), fallen_from=int(np.argmax(~alive)) if not alive.all() else -1,
                 limited_rows=int(((st_ld & rf.LIMITED) != 0).sum()), clipped_rows=int(((st_ld & ro.CLIPPED) != 0).sum()))
        for name, (cols, bound) in fc.ROW_GROUPS.items():
            floor = fc.dist(w64[1][:, cols], wld[1][:, cols])
            e[name] = dict(floor=floor, gate=fc.state_gate(floor, bound, K), error=fc.dist(rows[b, :n, cols], wld[1][:, cols]))
        floor = fc.dist(w64[4], wld[4])
        e["state"] = dict(floor=floor, gate=fc.state_gate(floor, fc.RATE, K), error=fc.dist(state[b], wld[4]))
        gate_fa = np.zeros(n)
        for c in sorted(set(int(v) for v in cnt)):
            m = cnt == c
            Kc = float(Krow[m & alive].max()) if (m & alive).any() else 1.0
            for name, (cols, factor) in fc.FEET_GROUPS.items():
                floor = fc.dist(w64[2][m][:, cols], wld[2][m][:, cols])
                e["%s_stance%d" % (name, c)] = dict(floor=floor, gate=fc.feet_gate(floor, factor, Kc), cond=Kc, rows=int(m.sum()),
                                                    error=fc.dist(frows[b, :n][m][:, cols], wld[2][m][:, cols]))
            gate_fa[m] = e["f_a_stance%d" % c]["gate"]
        # no row within its gate of a threshold: the feedback clips and the limit (in any step of the tick), dev_max and tilt_max
        near = np.asarray(det["near"], F64)
        row_floor = np.abs(np.asarray(w64[2][:, 1:13], LD) - wld[2][:, 1:13]).max(axis=1).astype(F64)      # the float64 floor of the row's own forces
        row_gate = np.maximum(Krow * fc.E_RHS, 8 * row_floor)
        assert (near[alive] > row_gate[alive]).all(), np.nonzero(alive & ~(near > row_gate))[0]
        seen = np.concatenate([[True], alive[:-1]])                                    # rows whose |e| and tilt were compared with the limits
        apart = np.minimum(np.abs(np.asarray(wld[1][:, 17], F64) - DEV_MAX), np.abs(np.asarray(wld[1][:, 18], F64) - TILT_MAX))
        assert (apart[seen] > e["norms"]["gate"]).all()
        e["nearest_threshold"] = dict(feet_and_clips=float((near[alive] / row_gate[alive]).min()), fall=float(apart[seen].min()))
        assert np.array_equal(status[b, :n], st_ld) and word[b] == wld[6] and count[b] == wld[5]
        assert np.array_equal((status[b, :n] & rf.TWO_STANCE) != 0, cnt == 2) and not (status[b, :n] & (rf.NO_STANCE | ro.PENDING)).any()
        if feet == "limited":
            f = frows[b, :n, 1:13].reshape(n, 4, 3)
            on = det["stance"] & alive[:, None]
            ok = (f[:, :, 2] >= 0) & (f[:, :, 2] <= 30.0) & (np.abs(f[:, :, 0]) <= 0.7 * f[:, :, 2]) & (np.abs(f[:, :, 1]) <= 0.7 * f[:, :, 2])
            assert ok[on].all() and 0 < e["limited_rows"] < n
        else:
            assert e["limited_rows"] == 0
        j = np.arange(n)
        acts = (COUNT_IN[b] + j >= PUSH_FROM) & (COUNT_IN[b] + j < PUSH_FROM + PUSH_TICKS) & alive
        assert np.array_equal((status[b, :n] & ro.PUSH) != 0, acts)
        frozen = ~alive
        assert (frows[b, :n][frozen][:, 13:16] == 0).all()
        entry["window%d" % b] = e
    fc.record("gpu_%s_%s_substeps%d" % (case.name, feet, sub), entry)
    assert sum(entry["window%d" % b]["clipped_rows"] for b in (1, 2)) > 0 or case.name == "walk"
    for e in entry.values():
        for name, v in e.items():
            if isinstance(v, dict) and "error" in v:
                assert v["error"] <= v["gate"], (case.name, feet, sub, name, v)


def one_window(case, b, params, **kw):
    args = dict(joint=case.joint[b:b + 1, :params.n_rows] if params.capacity == 0 else None, mass_scale=MASS_SCALE[b:b + 1], push=PUSH[b:b + 1],
                count=COUNT_IN[b:b + 1])
    args.update(kw)
    return case.P.rollout_feet(case.nodes[b:b + 1], T0[b:b + 1], params, **args)


def test_two_segments_with_the_carried_state_are_one_call(case):
    b, cut = 2, 300
    meas, rows, frows, status, state, count, word = case.got("limited", 3)
    first = one_window(case, b, case.params("limited", 3, n_rows=cut))
    p2 = case.params("limited", 3, first_row=cut, n_rows=N_ROWS - cut, init=False)
    second = one_window(case, b, p2, joint=case.joint[b:b + 1, cut:], state=first[4], count=first[5], word=first[6])
    for i, whole in enumerate((meas, rows, frows)):
        assert np.array_equal(bits(np.concatenate([first[i], second[i]], 1)), bits(whole[b:b + 1]))
    assert np.array_equal(np.concatenate([first[3], second[3]], 1), status[b:b + 1])
    assert np.array_equal(bits(second[4][0]), bits(state[b])) and second[5][0] == count[b] and second[6][0] == word[b]


def test_a_pending_word_sets_each_window_on_its_plan_at_its_first_rows(case):
    from qtos_amd import capi
    meas, rows, frows, status, state, count, word = case.got("limited", 3)
    p = case.params("limited", 3, init=False)
    assert not p.flags & capi.ROLLOUT_INIT
    got = case.run(p, word=np.full(B, capi.ROLLOUT_PENDING, np.int32))
    for i, whole in enumerate((meas, rows, frows)):
        assert np.array_equal(bits(got[i]), bits(whole))
    assert np.array_equal(got[3], status) and np.array_equal(bits(got[4]), bits(state)) and np.array_equal(got[5], count)
    assert got[6].tolist() == [capi.ROLLOUT_PENDING, word[1], word[2]]


def test_ring_mode_is_the_table(case):
    """Capacity 300, two appends of 200 rows from cursor 130: the first wraps inside its first tile, the second lies over the first's
    oldest rows.  The rings' rows are the table-mode rows of the same row numbers, to the bit."""
    from qtos_amd.stitcher import ring_rows
    cap, seg, b, cur0 = 300, 200, 2, 130
    table = one_window(case, b, case.params("limited", 1, n_rows=2 * seg))
    ring_m, ring_r, ring_f, ring_s = np.full((1, cap, 18), -7.5), np.full((1, cap, 20), -7.5), np.full((1, cap, 16), -7.5), np.full((1, cap), -7, np.int32)
    ring_j = np.full((1, cap, 37), np.nan)
    cursor, state, count, word = cur0, None, COUNT_IN[b:b + 1], None
    for i in range(2):
        at = (cursor + np.arange(seg)) % cap
        ring_j[0, at] = case.joint[b, i * seg:(i + 1) * seg]
        p = case.params("limited", 1, first_row=i * seg, n_rows=seg, capacity=cap, init=i == 0)
        ring_m, ring_r, ring_f, ring_s, state, count, word = one_window(case, b, p, joint=ring_j, cursor=np.array([cursor], np.int64), state=state,
                                                                        count=count, word=word, meas=ring_m, rows=ring_r, frows=ring_f, status=ring_s)
        if i == 0:
            free = np.setdiff1d(np.arange(cap), at)
            assert (ring_r[0, free] == -7.5).all() and (ring_s[0, free] == -7).all() and (ring_m[0, free] == -7.5).all() and (ring_f[0, free] == -7.5).all()
        cursor += seg
    for ring, tab in ((ring_m, table[0]), (ring_r, table[1]), (ring_f, table[2])):
        assert np.array_equal(bits(ring_rows(ring[0], cursor)), bits(tab[0, -cap:]))
    assert np.array_equal(ring_rows(ring_s[0], cursor), table[3][0, -cap:])
    assert np.array_equal(bits(state), bits(table[4])) and count[0] == table[5][0] and word[0] == table[6][0]


def test_tick_of_five_robots(case):
    """B = 5, one row each at a row index of its own, from the state the table's kernel carries there: the one-wave instantiation's
    rows are the table's rows, to the bit; and a full wave of it, and one row more (the 256-lane kernel)."""
    n, b = 5, 1
    first = np.array([1, 2, 100, TILE - 2, TILE - 1], np.int32)
    meas, rows, frows, status, state, count, word = case.got("limited", 3)
    nodes, t0 = np.repeat(case.nodes[b:b + 1], n, axis=0), np.repeat(T0[b:b + 1], n)
    shared = dict(mass_scale=np.repeat(MASS_SCALE[b], n), push=np.repeat(PUSH[b:b + 1], n, axis=0))
    upto = case.P.rollout_feet(nodes, t0, case.params("limited", 3), n_rows=first, joint=np.repeat(case.joint[b:b + 1], n, axis=0),
                               count=np.repeat(COUNT_IN[b], n), **shared)
    tick = case.P.rollout_feet(nodes, t0, case.params("limited", 3, n_rows=1, init=False), first_row=first, joint=case.joint[b, first][:, None, :],
                               state=upto[4], count=upto[5], word=upto[6], **shared)
    assert tick[2].shape == (n, 1, 16)
    for i, whole in enumerate((meas, rows, frows)):
        assert np.array_equal(bits(tick[i][:, 0]), bits(whole[b, first]))
    assert np.array_equal(tick[3][:, 0], status[b, first]) and tick[5].tolist() == (COUNT_IN[b] + first + 1).tolist()
    assert np.array_equal(bits(tick[4][-1]), bits(state[b]))                              # behind the last row: the table's carried state
    pre = one_window(case, b, case.params("limited", 3, n_rows=100))
    for m in (64, 65):
        part = one_window(case, b, case.params("limited", 3, first_row=100, n_rows=m, init=False), joint=case.joint[b:b + 1, 100:100 + m],
                          state=pre[4], count=pre[5], word=pre[6])
        for i, whole in enumerate((meas, rows, frows)):
            assert np.array_equal(bits(part[i][0]), bits(whole[b, 100:100 + m]))
        assert np.array_equal(part[3][0], status[b, 100:100 + m])


def test_device_form_on_a_held_up_stream_is_the_host_form(case):
    import torch
    dev = torch.device("cuda", 0)
    meas, rows, frows, status, state, count, word = case.got("limited", 3)
    p = case.params("limited", 3)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0, d_n = torch.as_tensor(T0, **f64), torch.as_tensor(COUNTS, device=dev)
    d_joint, d_ms, d_push = torch.as_tensor(np.array(case.joint), **f64), torch.as_tensor(MASS_SCALE, **f64), torch.as_tensor(PUSH, **f64)
    src = torch.as_tensor(case.nodes, **f64)
    side = torch.cuda.Stream(dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)              # (elementwise work: holds the stream up, loads no BLAS library)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        o_m, o_r, o_f = torch.full((B, N_ROWS, 18), -7.5, **f64), torch.full((B, N_ROWS, 20), -7.5, **f64), torch.full((B, N_ROWS, 16), -7.5, **f64)
        o_s = torch.full((B, N_ROWS), -7, dtype=torch.int32, device=dev)
        d_state, d_count, d_word = torch.as_tensor(STATE_IN, **f64), torch.as_tensor(COUNT_IN, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if stream is side:
                for _ in range(50):
                    busy.mul_(1.0001).clamp_(0.0, 1.0)
            d_nodes = src + 0.0
            r = case.P.lib.qtos_rollout_feet_device(case.P.h, B, C.byref(p), d_nodes.data_ptr(), d_t0.data_ptr(), None, d_n.data_ptr(), None,
                                                    d_joint.data_ptr(), d_ms.data_ptr(), d_push.data_ptr(), d_state.data_ptr(), d_count.data_ptr(),
                                                    d_word.data_ptr(), o_m.data_ptr(), o_r.data_ptr(), o_f.data_ptr(), o_s.data_ptr(),
                                                    C.c_void_p(stream.cuda_stream))
            assert r == 0, case.P.lib.qtos_last_error(case.P.h)
        stream.synchronize()
        assert np.array_equal(bits(o_m.cpu().numpy()), bits(meas)) and np.array_equal(bits(o_r.cpu().numpy()), bits(rows))
        assert np.array_equal(bits(o_f.cpu().numpy()), bits(frows))
        assert np.array_equal(o_s.cpu().numpy(), status) and np.array_equal(bits(d_state.cpu().numpy()), bits(state))
        assert np.array_equal(d_count.cpu().numpy(), count) and np.array_equal(d_word.cpu().numpy(), word)
    torch.cuda.synchronize()


@pytest.mark.parametrize("sub", [1, 3])
def test_without_gains_r_and_v_are_qtos_rollouts_own(case, sub):
    """Gains 0, ff_scale 1, no limit: df = 0 exactly, so r and v of every row, and of the carried state, are the bits of qtos_rollout's
    output on the same inputs; columns 13 .. 15 are 0 and f_a is the plan's force.  dev_max 0.5 m stops the heavy window, which falls
    without gains, at the same row in both kernels (|e| is made of r alone: the same bits); left to fall, its rotation -- an explicit
    step of w x I w -- overflows within 1.5 s, and 0 x inf is not 0: df = 0 holds for finite states."""
    from qtos_amd import capi
    from qtos_amd.config import INERTIA_PHYSICAL
    body = dict(inertia_b=INERTIA_PHYSICAL, substeps=sub, push_from=PUSH_FROM, push_ticks=PUSH_TICKS, dev_max=0.5)
    got = case.run(case.params("free", sub, body=body))
    plain = case.P.rollout(case.nodes, T0, capi.rollout_params(cfg=case.cfg, hz=case.hz, n_rows=N_ROWS, init=True, **body), n_rows=COUNTS, joint=case.joint,
                           mass_scale=MASS_SCALE, push=PUSH, state=STATE_IN, count=COUNT_IN, word=np.zeros(B, np.int32),
                           meas=np.full((B, N_ROWS, 18), -7.5), rows=np.full((B, N_ROWS, 20), -7.5), status=np.full((B, N_ROWS), -7, np.int32))
    for cols in (slice(0, 4), slice(7, 10)):
        assert np.array_equal(bits(got[1][:, :, cols]), bits(plain[1][:, :, cols]))
    assert np.array_equal(bits(got[0][:, :, 0:3]), bits(plain[0][:, :, 0:3])) and np.array_equal(bits(got[4][:, 0:6]), bits(plain[3][:, 0:6]))
    assert np.array_equal(got[5], plain[4]) and np.array_equal(got[6], plain[5])
    for b in (1, 2):
        n = int(COUNTS[b])
        assert (got[2][b, :n, 13:16] == 0).all() and np.array_equal(got[2][b, :n, 1:13], case.sample[b, :n, 25:37])
        assert np.array_equal(got[3][b, :n] & ~(64 | 128), plain[2][b, :n]) and not (got[3][b, :n] & 2).any()
    assert got[6].tolist() == [0, 0, 1]                                                   # the heavy window fell, in both


def test_argument_checks(case):
    cap = 300
    p = case.params("limited", 1, first_row=40, n_rows=200, capacity=cap, init=False)
    meas, rows, fr, st = np.zeros((1, cap, 18)), np.zeros((1, cap, 20)), np.zeros((1, cap, 16)), np.zeros((1, cap), np.int32)
    state, count, word = np.zeros((1, 13)), np.zeros(1, np.int64), np.zeros(1, np.int32)
    state[0, 9] = 1.0
    from qtos_amd import capi

    def call(**kw):
        a = dict(h=case.P.h, b=1, s=p, nodes=case.nodes[:1], t0=T0[:1], cur=np.array([0], np.int64), state=state.copy(), count=count.copy(),
                 word=word.copy(), meas=meas.copy(), rows=rows.copy(), fr=fr.copy(), st=st.copy())
        a.update(kw)
        ll = lambda v: None if v is None else v.ctypes.data_as(LLP)
        return case.P.lib.qtos_rollout_feet(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]), None,
                                            None, ll(a["cur"]), None, None, None, capi._dp(a["state"]), ll(a["count"]), capi._ip(a["word"]),
                                            capi._dp(a["meas"]), capi._dp(a["rows"]), capi._dp(a["fr"]), capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            setattr(s, key, v)
        return s
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null state": call(state=None), "null meas": call(meas=None), "null status": call(st=None), "ring without cursor": call(cur=None),
           "capacity < 0": call(s=params(capacity=-1)), "substeps 0": call(s=params(substeps=0)), "hz 0": call(s=params(hz=0.0)),
           "mass 0": call(s=params(mass=0.0)), "arm 0": call(s=params(arm=0.0)), "arm nan": call(s=params(arm=float("nan"))),
           "damping 0": call(s=params(damping=0.0)), "w_min 0": call(s=params(w_min=0.0)), "w_min 1.5": call(s=params(w_min=1.5)),
           "mu < 0": call(s=params(mu=-0.5)), "mu nan": call(s=params(mu=float("nan")))}
    assert all(v == -1 for v in got.values()), got
    assert b"qtos_rollout_feet: mu" in case.P.lib.qtos_last_error(case.P.h)
    call(s=params(substeps=0))
    assert b"qtos_rollout_feet: substeps" in case.P.lib.qtos_last_error(case.P.h)
    call(s=params(w_min=1.5))
    assert b"w_min" in case.P.lib.qtos_last_error(case.P.h)
    assert call() == 0 and call(rows=None) == 0 and call(fr=None) == 0 and call(s=params(w_min=1.0, mu=0.0, f_max=0.0)) == 0


def test_rollout_feet_from_plain_c(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "rolloutfeet_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "rolloutfeet_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[2] == "rollout_feet_null=-1 rollout_feet_device_null=-1"
    assert lines[3].startswith("bad_args=" + ",".join(["-1"] * 8) + " reason=qtos_rollout_feet: mu")
    assert lines[4] == "plan rc=0 status=0,0"
    kv = dict(t.split("=") for t in lines[5].split()[1:])
    assert kv["rc"] == "0,0" and int(kv["mismatches"]) == 0 and int(kv["two_stance"]) > 800          # (of 2 x 800 rows: a trot)
    for i, limit in ((6, 0), (7, 1)):
        kv = dict(t.split("=") for t in lines[i].split()[1:])
        assert int(kv["limit"]) == limit and int(kv["rc"]) == 0 and int(kv["mismatches"]) == 0 and float(kv["miss_t"]) > 0
        assert (int(kv["limited"]) > 0) == bool(limit)


def test_feet_switch_of_shifted_windows_is_the_rule_segment_by_segment():
    """B = 4, three replans of 420 rows into rings of 1000 (the third append wraps), joints, track, feedback and the rollout through
    the feet on (the limited setting; window 3 pushed): behind every replan the measured ring's, the rollout ring's and the feet
    ring's rows of the segment are the longdouble rule's, applied segment by segment with the state, count and word it carries
    itself, at the gates above; the status words are the rule's.  Without ``feet`` nothing of it is allocated, the feet kernel is
    never queued (its entry point is replaced by one that raises) and two such sets give the same plans, rings, cursors and clocks --
    the plain path is deterministic and never reaches the new kernel; that its bits are the parent's is what the tests it had keep
    holding (tests/test_gpu_rollout.py's ShiftedWindows case among them)."""
    import torch
    from oracle import splines as sp
    from qtos_amd import capi, rollout as ro, rollout_feet as rf, workloads
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
    push[3] = (3.0, 1.5, 0.0, 0.0, 0.0, 0.05)
    body = dict(inertia_b=INERTIA_PHYSICAL, substeps=2, push_from=500, push_ticks=200, dev_max=0.5, tilt_max=1.0, **fc.GAINS)
    scale = np.array([1.0, 1.1, 1.0, 1.0])
    common = dict(advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(tau_max=3.0), track=dict(delay=0, rule="clean"), feedback=dict(cfg=cfg))
    try:
        plain = []
        real = P.lib.qtos_rollout_feet_device
        for _ in range(2):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], stream=torch.cuda.Stream(), rollout=dict(cfg=cfg, mass_scale=scale, push=push, rows=True, **body),
                               **common)
            assert W._feet is None and not hasattr(W, "rollout_feet_traj")
            with pytest.raises(RuntimeError):
                W.rollout_feet_rows(0)

            def never(*a):
                raise AssertionError("the feet kernel was queued")
            P.lib.qtos_rollout_feet_device = never
            try:
                for _ in range(3):
                    W.replan()
                W.finish()
                torch.cuda.synchronize()
            finally:
                P.lib.qtos_rollout_feet_device = real
            plain.append([host(W.nodes), host(W.traj), host(W.meas_traj), host(W.rollout_traj), host(W.rollout_status), host(W.cursor), host(W.t0)])
        for a, b in zip(*plain):
            assert a.tobytes() == b.tobytes()
        W = ShiftedWindows(P, start, goal - start[:, 0:3], stream=torch.cuda.Stream(),
                           rollout=dict(cfg=cfg, mass_scale=scale, push=push, rows=True, feet=dict(FEET["limited"]), **body), **common)
        assert W._feet.mu == 0.7 and W._feet.feet_flags == capi.FEET_LIMIT and W.rollout_feet_traj.shape == (nb, cap, 16)
        W.replan()
        torch.cuda.synchronize()
        assert (host(W.rollout_word) == capi.ROLLOUT_PENDING).all() and (host(W.rollout_count) == 0).all()    # no plan to hand over from yet
        rp, fp = ro.RolloutParams(cfg, **body), rf.FeetParams(cfg, **FEET["limited"])
        carried = [dict(state=None, count=0, word=ro.PENDING) for _ in range(nb)]
        c64 = [dict(state=None, count=0, word=ro.PENDING) for _ in range(nb)]
        entry = {}
        for i in range(3):
            h_nodes, h_t0, cur = host(W.nodes), host(W.t0), host(W.cursor)
            W.replan()
            torch.cuda.synchronize()
            assert (host(W.row) == seg).all() and (host(W.cursor) == cur + seg).all()
            at = (cur[0] + np.arange(seg)) % cap
            meas, rows, fr, st = host(W.meas_traj)[:, at], host(W.rollout_traj)[:, at], host(W.rollout_feet_traj)[:, at], host(W.rollout_status)[:, at]
            joint, _ = P.joint_rows(h_nodes, h_t0, capi.joint_params(hz=1000.0, n_rows=seg, tau_max=3.0))
            for b in range(nb):
                out = {}
                for dt, cs in ((LD, carried), (F64, c64)):
                    c = cs[b]
                    out[dt] = rf.rollout_feet_rows(L, h_nodes[b], h_t0[b], 1000.0, 0, seg, rp, fp, state=c["state"], count=c["count"], word=c["word"],
                                                   mass_scale=scale[b], push=push[b], joint=joint[b], dtype=dt, detail=True)
                    c["state"], c["count"], c["word"] = out[dt][4], out[dt][5], out[dt][6]
                wld, w64 = out[LD], out[F64]
                Krow = row_conditions(w64[7]["M"])
                K = float(Krow.max())
                e = dict(cond=K, limited=int(((wld[3] & rf.LIMITED) != 0).sum()))
                for name, got, col, bound in (("pos", meas[b, :, 0:3], (0, slice(0, 3)), fc.POS), ("euler", meas[b, :, 3:6], (0, slice(3, 6)), fc.EULER),
                                              ("rate", rows[b, :, 7:13], (1, slice(7, 13)), fc.RATE)):
                    floor = fc.dist(w64[col[0]][:, col[1]], wld[col[0]][:, col[1]])
                    e[name] = dict(floor=floor, gate=fc.state_gate(floor, bound, K), error=fc.dist(got, wld[col[0]][:, col[1]]))
                floor = fc.dist(w64[2][:, 1:13], wld[2][:, 1:13])
                e["f_a"] = dict(floor=floor, gate=fc.feet_gate(floor, 1.0, K), error=fc.dist(fr[b, :, 1:13], wld[2][:, 1:13]))
                floor = fc.dist(w64[2][:, 13:16], wld[2][:, 13:16])
                e["missing"] = dict(floor=floor, gate=fc.feet_gate(floor, 4.0, K), error=fc.dist(fr[b, :, 13:16], wld[2][:, 13:16]))
                near = np.asarray(wld[7]["near"], F64)
                row_floor = np.abs(np.asarray(w64[2][:, 1:13], LD) - wld[2][:, 1:13]).max(axis=1).astype(F64)
                alive = (wld[3] & 3) == 0
                assert (near[alive] > np.maximum(Krow * fc.E_RHS, 8 * row_floor)[alive]).all(), (i, b)
                assert np.array_equal(bits(meas[b, :, 6:18]), bits(joint[b, :, 1:13])) and np.array_equal(st[b], wld[3]), (i, b)
                assert np.array_equal(bits(fr[b, :, 0]), bits(rows[b, :, 0]))
                for name, v in e.items():
                    if isinstance(v, dict):
                        assert v["error"] <= v["gate"], (i, b, name, v)
                entry["replan%d_window%d" % (i, b)] = e
            assert host(W.rollout_count).tolist() == [(i + 1) * seg] * nb
        W.finish()
        torch.cuda.synchronize()
        f3 = W.rollout_feet_rows(3)
        r3, s3 = W.rollout_rows(3)
        assert f3.shape == (cap, 16) and np.array_equal(bits(f3[:, 0]), bits(r3[:, 0]))
        assert sum(e["limited"] for e in entry.values()) > 0
        fc.record("gpu_shifted_windows", entry)
    finally:
        P.close()
