"""The kernel of the rollout with the force QP on the MI355X (pytest -m gpu): k_rollout_qp against the longdouble rule
(qtos_amd/rollout_qp.py), its exact columns, table against ring, the tick, a held-up side stream against the host form, the rows
before the first limit against qtos_rollout_feet's, feasibility, the argument checks and the QP switch of ShiftedWindows against the
rule applied segment by segment.  (The call from plain C: tests/test_rolloutqp_caller.py.)

Shapes: tests/rollout_cases.py's, the smallest at which the chain can go wrong -- B = 3 windows x 549 rows (two full 256-row tiles
and a partial one, rows past the horizon), counts 0 / 256 / 549, window 2 1.3 x as heavy and pushed, substeps 1 and 3, dev_max
0.15 m, tilt_max 0.3 rad.  Plans: the golden walk, and the device's own trot as tests/test_gpu_rollout_feet.py plans it.  Settings,
gates, the pool of the limited rows' floors and the asserted conditions: tests/rollout_qp_cases.py.  Every case's rules are made
before the first comparison (the pool needs them all); they are made once and shared by the tests.

Exact, on every row, under the conditions asserted from the longdouble rule (share of rows left out: 0): time stamps, joint
columns, counts, carried words, status words (LIMITED and CAP among them) and the step counts of the tick's first step."""
import ctypes as C

import numpy as np
import pytest

import rollout_qp_cases as qc
from conftest import load_gv
from rollout_cases import B, COUNT_IN, COUNTS, F64, LD, MASS_SCALE, N_ROWS, PUSH, T0, TILE

pytestmark = pytest.mark.gpu
STATE_IN = np.arange(B * 13, dtype=F64).reshape(B, 13) * 0.01 + 0.5        # (the INIT flag replaces it where a window has rows)
LLP = C.POINTER(C.c_longlong)
NAMES, SUBS = ("walk", "trot"), (1, 3)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Case:
    """One plan: its planner, nodes, the joint table of B windows; kernel results and rules are made once per substeps."""

    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name, self.hz = name, qc.SETTINGS[name]["hz"]
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
        self._got, self.want = {}, {}

    def params(self, sub, **kw):
        from qtos_amd import capi
        args = dict(cfg=self.cfg, hz=self.hz, n_rows=N_ROWS, init=True)
        args.update(kw)
        return capi.rollout_qp_params(**args, **qc.feet_kw(self.name), **qc.body_kw(sub))

    def feet_params(self, sub, **kw):
        from qtos_amd import capi
        args = dict(cfg=self.cfg, hz=self.hz, n_rows=N_ROWS, init=True)
        args.update(kw)
        return capi.rollout_feet_params(**args, **qc.feet_kw(self.name), **qc.body_kw(sub))

    def base_args(self, mcols=18):
        return dict(n_rows=COUNTS, joint=self.joint, mass_scale=MASS_SCALE, push=PUSH, state=STATE_IN, count=COUNT_IN, word=np.zeros(B, np.int32),
                    meas=np.full((B, N_ROWS, mcols), -7.5), rows=np.full((B, N_ROWS, 20), -7.5), frows=np.full((B, N_ROWS, 16), -7.5),
                    status=np.full((B, N_ROWS), -7, np.int32))

    def got(self, sub):
        """The base call: per-window counts, a state, count and word that stand, the tables pre-filled."""
        if sub not in self._got:
            self._got[sub] = self.P.rollout_qp(self.nodes, T0, self.params(sub), qrows=np.full((B, N_ROWS, 8), -7.5), **self.base_args())
        return self._got[sub]


_cases = {}


def all_cases():
    """Both plans with their rules at both substeps, made at the first call: the pool's floors are over all of them."""
    if not _cases:
        for name in NAMES:
            _cases[name] = c = Case(name)
            for sub in SUBS:
                c.want[sub] = [None] + [qc.window_rules(c.L, c.cfg, c.nodes[b], name, sub, b, joint=c.joint[b]) for b in (1, 2)]
                for b in (1, 2):
                    qc.pool_add("gpu", c.want[sub][b][F64], c.want[sub][b][LD])
    return _cases


@pytest.fixture(params=NAMES)
def case(request):
    return all_cases()[request.param]


@pytest.fixture(scope="module", autouse=True)
def _close_planners():
    yield
    for c in _cases.values():
        c.P.close()
    _cases.clear()


@pytest.mark.parametrize("sub", SUBS)
def test_kernel_against_the_rule(case, sub):
    from qtos_amd import rollout as ro, rollout_qp as rq
    meas, rows, frows, qrows, status, state, count, word = case.got(sub)
    s_ = qc.SETTINGS[case.name]
    assert N_ROWS > 2 * TILE and (N_ROWS - 1) / case.hz > case.L.T                           # a partial third tile, rows past the horizon
    assert np.array_equal(bits(state[0]), bits(STATE_IN[0])) and count[0] == COUNT_IN[0] and word[0] == 0     # no rows: kept
    assert (frows[0] == -7.5).all() and (rows[0] == -7.5).all() and (qrows[0] == -7.5).all() and count[1:].tolist() == [TILE, 2 + N_ROWS]
    entry = {}
    for b in (1, 2):
        n = int(COUNTS[b])
        w64, wld = case.want[sub][b][F64], case.want[sub][b][LD]
        det = wld[8]
        for tab in (meas, rows, frows, qrows):
            assert (tab[b, n:] == -7.5).all()
        assert (status[b, n:] == -7).all()
        assert np.array_equal(bits(rows[b, :n, 0]), bits(case.sample[b, :n, 0])) and np.array_equal(bits(frows[b, :n, 0]), bits(rows[b, :n, 0]))
        assert np.array_equal(bits(meas[b, :n, 6:18]), bits(case.joint[b, :n, 1:13]))                          # the joint table's angles
        assert np.array_equal(bits(meas[b, :n, 0:6]), bits(rows[b, :n, 1:7]))
        st_ld, alive = wld[4], det["alive"]
        assert not (st_ld & (ro.NONFINITE | ro.GIMBAL)).any()
        e, gate_fa = qc.compare(rows[b, :n], frows[b, :n], qrows[b, :n], state[b], w64, wld, qc.feet_of(case.name), "gpu")
        qc.assert_conditions(wld, w64, gate_fa, 1e-3, e)
        # exact: the status words, the carried word and count, the steps and the active rows of the first step
        assert np.array_equal(status[b, :n], st_ld) and word[b] == wld[7] and count[b] == wld[6]
        assert np.array_equal(qrows[b, :n, 0], np.asarray(wld[3][:, 0], F64)) and np.array_equal(qrows[b, :n, 7], np.asarray(wld[3][:, 7], F64))
        assert np.array_equal(np.asarray(w64[3][:, [0, 7]], F64), np.asarray(wld[3][:, [0, 7]], F64)) and np.array_equal(w64[8]["steps"], det["steps"])
        assert not (status[b, :n] & rq.CAP).any() and 0 < e["limited_rows"] < n
        # feasibility: every alive stance force strictly inside the limits
        f = frows[b, :n, 1:13].reshape(n, 4, 3)
        on = det["stance"] & alive[:, None]
        ok = (f[:, :, 2] > 0) & (f[:, :, 2] < s_["f_max"]) & (np.abs(f[:, :, 0]) < s_["mu"] * f[:, :, 2]) & (np.abs(f[:, :, 1]) < s_["mu"] * f[:, :, 2])
        assert ok[on].all() and (qrows[b, :n, 3][alive & (det["stance"].sum(axis=1) > 0)] > 0).all()
        frozen = ~alive
        assert (frows[b, :n][frozen][:, 13:16] == 0).all() and (qrows[b, :n][frozen] == 0).all()
        entry["window%d" % b] = e
    qc.record("gpu_%s_substeps%d" % (case.name, sub), entry)
    qc.assert_within(entry, (case.name, sub))


def one_window(case, b, params, **kw):
    args = dict(joint=case.joint[b:b + 1, :params.n_rows] if params.capacity == 0 else None, mass_scale=MASS_SCALE[b:b + 1], push=PUSH[b:b + 1],
                count=COUNT_IN[b:b + 1])
    args.update(kw)
    return case.P.rollout_qp(case.nodes[b:b + 1], T0[b:b + 1], params, **args)


def test_ring_mode_is_the_table(case):
    """Capacity 300, two appends of 200 rows from cursor 130: the first wraps inside its first tile, the second lies over the first's
    oldest rows.  The rings' rows are the table-mode rows of the same row numbers, to the bit."""
    from qtos_amd.stitcher import ring_rows
    cap, seg, b, cur0 = 300, 200, 1, 130
    table = one_window(case, b, case.params(1, n_rows=2 * seg))
    rings = [np.full((1, cap, c), -7.5) for c in (18, 20, 16, 8)]
    ring_s = np.full((1, cap), -7, np.int32)
    ring_j = np.full((1, cap, 37), np.nan)
    cursor, state, count, word = cur0, None, COUNT_IN[b:b + 1], None
    for i in range(2):
        at = (cursor + np.arange(seg)) % cap
        ring_j[0, at] = case.joint[b, i * seg:(i + 1) * seg]
        p = case.params(1, first_row=i * seg, n_rows=seg, capacity=cap, init=i == 0)
        out = one_window(case, b, p, joint=ring_j, cursor=np.array([cursor], np.int64), state=state, count=count, word=word, meas=rings[0],
                         rows=rings[1], frows=rings[2], qrows=rings[3], status=ring_s)
        rings, ring_s, state, count, word = list(out[0:4]), out[4], out[5], out[6], out[7]
        if i == 0:
            free = np.setdiff1d(np.arange(cap), at)
            assert all((r[0, free] == -7.5).all() for r in rings) and (ring_s[0, free] == -7).all()
        cursor += seg
    for ring, tab in zip(rings, table[0:4]):
        assert np.array_equal(bits(ring_rows(ring[0], cursor)), bits(tab[0, -cap:]))
    assert np.array_equal(ring_rows(ring_s[0], cursor), table[4][0, -cap:])
    assert np.array_equal(bits(state), bits(table[5])) and count[0] == table[6][0] and word[0] == table[7][0]
    assert (table[4] & 256).any()


def test_tick_of_five_robots(case):
    """B = 5, one row each at a row index of its own, from the state the table's kernel carries there: the one-wave instantiation's
    rows are the table's rows, to the bit; and a full wave of it, and one row more (the 256-lane kernel)."""
    n, b = 5, 1
    first = np.array([1, 2, 100, TILE - 2, TILE - 1], np.int32)
    whole = case.got(3)
    nodes, t0 = np.repeat(case.nodes[b:b + 1], n, axis=0), np.repeat(T0[b:b + 1], n)
    shared = dict(mass_scale=np.repeat(MASS_SCALE[b], n), push=np.repeat(PUSH[b:b + 1], n, axis=0))
    upto = case.P.rollout_qp(nodes, t0, case.params(3), n_rows=first, joint=np.repeat(case.joint[b:b + 1], n, axis=0), count=np.repeat(COUNT_IN[b], n),
                             **shared)
    tick = case.P.rollout_qp(nodes, t0, case.params(3, n_rows=1, init=False), first_row=first, joint=case.joint[b, first][:, None, :],
                             state=upto[5], count=upto[6], word=upto[7], **shared)
    assert tick[3].shape == (n, 1, 8)
    for i in range(4):
        assert np.array_equal(bits(tick[i][:, 0]), bits(whole[i][b, first]))
    assert np.array_equal(tick[4][:, 0], whole[4][b, first]) and tick[6].tolist() == (COUNT_IN[b] + first + 1).tolist()
    assert np.array_equal(bits(tick[5][-1]), bits(whole[5][b]))                           # behind the last row: the table's carried state
    pre = one_window(case, b, case.params(3, n_rows=100))
    for m in (64, 65):
        part = one_window(case, b, case.params(3, first_row=100, n_rows=m, init=False), joint=case.joint[b:b + 1, 100:100 + m],
                          state=pre[5], count=pre[6], word=pre[7])
        for i in range(4):
            assert np.array_equal(bits(part[i][0]), bits(whole[i][b, 100:100 + m]))
        assert np.array_equal(part[4][0], whole[4][b, 100:100 + m])


def test_device_form_on_a_held_up_stream_is_the_host_form(case):
    import torch
    dev = torch.device("cuda", 0)
    meas, rows, frows, qrows, status, state, count, word = case.got(3)
    p = case.params(3)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0, d_n = torch.as_tensor(T0, **f64), torch.as_tensor(COUNTS, device=dev)
    d_joint, d_ms, d_push = torch.as_tensor(np.array(case.joint), **f64), torch.as_tensor(MASS_SCALE, **f64), torch.as_tensor(PUSH, **f64)
    src = torch.as_tensor(case.nodes, **f64)
    side = torch.cuda.Stream(dev)
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)              # (elementwise work: holds the stream up, loads no BLAS library)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        o = [torch.full((B, N_ROWS, c), -7.5, **f64) for c in (18, 20, 16, 8)]
        o_s = torch.full((B, N_ROWS), -7, dtype=torch.int32, device=dev)
        d_state, d_count, d_word = torch.as_tensor(STATE_IN, **f64), torch.as_tensor(COUNT_IN, device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            if stream is side:
                for _ in range(50):
                    busy.mul_(1.0001).clamp_(0.0, 1.0)
            d_nodes = src + 0.0
            r = case.P.lib.qtos_rollout_qp_device(case.P.h, B, C.byref(p), d_nodes.data_ptr(), d_t0.data_ptr(), None, d_n.data_ptr(), None,
                                                  d_joint.data_ptr(), d_ms.data_ptr(), d_push.data_ptr(), d_state.data_ptr(), d_count.data_ptr(),
                                                  d_word.data_ptr(), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o_s.data_ptr(),
                                                  C.c_void_p(stream.cuda_stream))
            assert r == 0, case.P.lib.qtos_last_error(case.P.h)
        stream.synchronize()
        for t, want in zip(o, (meas, rows, frows, qrows)):
            assert np.array_equal(bits(t.cpu().numpy()), bits(want))
        assert np.array_equal(o_s.cpu().numpy(), status) and np.array_equal(bits(d_state.cpu().numpy()), bits(state))
        assert np.array_equal(d_count.cpu().numpy(), count) and np.array_equal(d_word.cpu().numpy(), word)
    torch.cuda.synchronize()


@pytest.mark.parametrize("sub", SUBS)
def test_rows_before_the_first_limit_are_qtos_rollout_feets(case, sub):
    """Before the first LIMITED row every step took the fit path: meas, rows, frows and the status words are qtos_rollout_feet's
    without QTOS_FEET_LIMIT on the same inputs, to the bit, and so is the state entering that row (r, v, q of its row)."""
    from qtos_amd import rollout_qp as rq
    got = case.got(sub)
    args = case.base_args()
    plain = case.P.rollout_feet(case.nodes, T0, case.feet_params(sub), **args)
    for b in (1, 2):
        n = int(COUNTS[b])
        lim = np.nonzero(got[4][b, :n] & rq.LIMITED)[0]
        k = int(lim[0]) if len(lim) else n
        assert 0 < k < n
        for i in range(3):
            assert np.array_equal(bits(got[i][b, :k]), bits(plain[i][b, :k]))
        assert np.array_equal(got[4][b, :k], plain[3][b, :k]) and (got[3][b, :k][:, [0, 1, 2, 4, 5, 6]] == 0).all()
        assert np.array_equal(bits(got[1][b, k, 0:19]), bits(plain[1][b, k, 0:19]))             # the state entering the first limited row


def test_argument_checks(case):
    cap = 300
    p = case.params(1, first_row=40, n_rows=200, capacity=cap, init=False)
    meas, rows, fr, qr, st = np.zeros((1, cap, 18)), np.zeros((1, cap, 20)), np.zeros((1, cap, 16)), np.zeros((1, cap, 8)), np.zeros((1, cap), np.int32)
    state, count, word = np.zeros((1, 13)), np.zeros(1, np.int64), np.zeros(1, np.int32)
    state[0, 9] = 1.0
    from qtos_amd import capi

    def call(**kw):
        a = dict(h=case.P.h, b=1, s=p, nodes=case.nodes[:1], t0=T0[:1], cur=np.array([0], np.int64), state=state.copy(), count=count.copy(),
                 word=word.copy(), meas=meas.copy(), rows=rows.copy(), fr=fr.copy(), qr=qr.copy(), st=st.copy())
        a.update(kw)
        ll = lambda v: None if v is None else v.ctypes.data_as(LLP)
        return case.P.lib.qtos_rollout_qp(a["h"], a["b"], None if a["s"] is None else C.byref(a["s"]), capi._dp(a["nodes"]), capi._dp(a["t0"]), None,
                                          None, ll(a["cur"]), None, None, None, capi._dp(a["state"]), ll(a["count"]), capi._ip(a["word"]),
                                          capi._dp(a["meas"]), capi._dp(a["rows"]), capi._dp(a["fr"]), capi._dp(a["qr"]), capi._ip(a["st"]))

    def params(**kw):
        s = p.copy()
        for key, v in kw.items():
            setattr(s, key, v)
        return s
    nan = float("nan")
    got = {"null planner": call(h=None), "B = 0": call(b=0), "null params": call(s=None), "null nodes": call(nodes=None),
           "null state": call(state=None), "null meas": call(meas=None), "null status": call(st=None), "ring without cursor": call(cur=None),
           "capacity < 0": call(s=params(capacity=-1)), "substeps 0": call(s=params(substeps=0)), "hz 0": call(s=params(hz=0.0)),
           "mass 0": call(s=params(mass=0.0)), "arm 0": call(s=params(arm=0.0)), "damping 0": call(s=params(damping=0.0)),
           "w_min 1.5": call(s=params(w_min=1.5)), "mu 0": call(s=params(mu=0.0)), "mu nan": call(s=params(mu=nan)), "f_max 0": call(s=params(f_max=0.0)),
           "f_max nan": call(s=params(f_max=nan)), "mu_end 0": call(s=params(mu_end=0.0)), "mu_end nan": call(s=params(mu_end=nan)),
           "max_iter 0": call(s=params(max_iter=0)), "max_iter 26": call(s=params(max_iter=26)), "act_tol nan": call(s=params(act_tol=nan))}
    assert all(v == -1 for v in got.values()), got
    assert b"qtos_rollout_qp: act_tol" in case.P.lib.qtos_last_error(case.P.h)
    for kw, reason in ((dict(substeps=0), b"qtos_rollout_qp: substeps"), (dict(w_min=1.5), b"qtos_rollout_qp: w_min"), (dict(mu=0.0), b"qtos_rollout_qp: mu is"),
                       (dict(f_max=0.0), b"qtos_rollout_qp: f_max"), (dict(mu_end=0.0), b"qtos_rollout_qp: mu_end"), (dict(max_iter=26), b"qtos_rollout_qp: max_iter")):
        call(s=params(**kw))
        assert reason in case.P.lib.qtos_last_error(case.P.h), (kw, case.P.lib.qtos_last_error(case.P.h))
    assert call() == 0 and call(rows=None) == 0 and call(fr=None) == 0 and call(qr=None) == 0 and call(s=params(feet_flags=1)) == 0


def test_qp_switch_of_shifted_windows_is_the_rule_segment_by_segment():
    """B = 4, three replans of 420 rows into rings of 1000 (the third append wraps), joints, track, feedback and the rollout with
    limit="qp" (window 3 pushed): behind every replan the measured ring's, the rollout ring's, the feet ring's and the solve ring's
    rows of the segment are the longdouble rule's, applied segment by segment with the state, count and word it carries itself, at
    the gates of tests/rollout_qp_cases.py (a pool of its own segments); the status words are the rule's, and the state the device carries
    behind the last replan is the rule's behind its last segment.  With limit=True and without ``feet`` the new entry
    point is never queued (it is replaced by one that raises) and nothing of it is allocated."""
    import torch
    from oracle import splines as sp
    from qtos_amd import capi, rollout as ro, rollout_qp as rq, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import INERTIA_PHYSICAL, PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    import rollout_feet_cases as fc
    nb, cap, seg = 4, 1000, 420
    cfg = PlannerConfig.knots100(gait="trot")
    L = sp.layout(cfg)
    start, goal = workloads.flat_goals(nb, seed=7)
    P = Planner(cfg, max_batch=nb)
    host = lambda t: t.cpu().numpy().copy()
    push = np.zeros((nb, 6))
    push[3] = (3.0, 1.5, 0.0, 0.0, 0.0, 0.05)
    body = dict(inertia_b=INERTIA_PHYSICAL, substeps=2, push_from=500, push_ticks=200, dev_max=0.5, tilt_max=1.0, **fc.GAINS)
    feet = dict(mu=0.7, f_max=30.0, damping=1e-2)
    scale = np.array([1.0, 1.1, 1.0, 1.0])
    common = dict(advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(tau_max=3.0), track=dict(delay=0, rule="clean"), feedback=dict(cfg=cfg))
    try:
        real = P.lib.qtos_rollout_qp_device

        def never(*a):
            raise AssertionError("the QP rollout kernel was queued")
        for extra in (dict(), dict(feet=dict(limit=True, **feet)), dict(feet=dict(limit=False, **feet))):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], stream=torch.cuda.Stream(), rollout=dict(cfg=cfg, mass_scale=scale, push=push, rows=True, **body, **extra),
                               **common)
            assert not hasattr(W, "rollout_qp_traj") and not W._feet_qp
            with pytest.raises(RuntimeError):
                W.rollout_qp_rows(0)
            P.lib.qtos_rollout_qp_device = never
            try:
                for _ in range(2):
                    W.replan()
                W.finish()
                torch.cuda.synchronize()
            finally:
                P.lib.qtos_rollout_qp_device = real
        W = ShiftedWindows(P, start, goal - start[:, 0:3], stream=torch.cuda.Stream(),
                           rollout=dict(cfg=cfg, mass_scale=scale, push=push, rows=True, feet=dict(limit="qp", mu_end=1e-6, act_tol=1e-3, max_iter=25, **feet), **body),
                           **common)
        assert W._feet.mu == 0.7 and W._feet.max_iter == 25 and W.rollout_qp_traj.shape == (nb, cap, 8) and W.rollout_feet_traj.shape == (nb, cap, 16)
        W.replan()
        torch.cuda.synchronize()
        assert (host(W.rollout_word) == capi.ROLLOUT_PENDING).all() and (host(W.rollout_count) == 0).all()    # no plan to hand over from yet
        rp, fp = ro.RolloutParams(cfg, **body), rq.QpFeetParams(cfg, **feet)
        carried = {dt: [dict(state=None, count=0, word=ro.PENDING) for _ in range(nb)] for dt in (LD, F64)}
        segments = []
        for i in range(3):
            h_nodes, h_t0, cur = host(W.nodes), host(W.t0), host(W.cursor)
            W.replan()
            torch.cuda.synchronize()
            assert (host(W.row) == seg).all() and (host(W.cursor) == cur + seg).all()
            at = (cur[0] + np.arange(seg)) % cap
            tabs = [host(t)[:, at] for t in (W.meas_traj, W.rollout_traj, W.rollout_feet_traj, W.rollout_qp_traj, W.rollout_status)]
            joint, _ = P.joint_rows(h_nodes, h_t0, capi.joint_params(hz=1000.0, n_rows=seg, tau_max=3.0))
            for b in range(nb):
                out = {}
                for dt in (LD, F64):
                    c = carried[dt][b]
                    out[dt] = rq.rollout_qp_rows(L, h_nodes[b], h_t0[b], 1000.0, 0, seg, rp, fp, state=c["state"], count=c["count"], word=c["word"],
                                                 mass_scale=scale[b], push=push[b], joint=joint[b], dtype=dt, detail=True, stop_tests=dt is LD)
                    c["state"], c["count"], c["word"] = out[dt][5], out[dt][6], out[dt][7]
                qc.pool_add("gpu_shifted_windows", out[F64], out[LD])
                segments.append((i, b, [t[b] for t in tabs], joint[b], out))
            assert host(W.rollout_count).tolist() == [(i + 1) * seg] * nb
        carried_state = host(W.rollout_state)                                             # behind the last replan: the last segment's
        entry = {}
        for i, b, (meas, rows, fr, qr, st), joint, out in segments:
            wld, w64 = out[LD], out[F64]
            e, gate_fa = qc.compare(rows, fr, qr, carried_state[b] if i == 2 else None, w64, wld, qc.Feet(**feet), "gpu_shifted_windows")
            qc.assert_conditions(wld, w64, gate_fa, 1e-3, e)
            floor = fc.dist(w64[0][:, 0:6], wld[0][:, 0:6])
            e["meas"] = dict(floor=floor, gate=fc.state_gate(max(floor, qc.POOLS["gpu_shifted_windows"].get("euler", 0.0)), fc.EULER, e["cond"]), error=fc.dist(meas[:, 0:6], wld[0][:, 0:6]))
            assert np.array_equal(bits(meas[:, 6:18]), bits(joint[:, 1:13])) and np.array_equal(st, wld[4]), (i, b)
            assert np.array_equal(bits(fr[:, 0]), bits(rows[:, 0])) and np.array_equal(qr[:, 0], np.asarray(wld[3][:, 0], F64))
            entry["replan%d_window%d" % (i, b)] = e
        W.finish()
        torch.cuda.synchronize()
        q3, f3 = W.rollout_qp_rows(3), W.rollout_feet_rows(3)
        assert q3.shape == (cap, 8) and f3.shape == (cap, 16)
        assert sum(e["limited_rows"] for e in entry.values()) > 0
        qc.record("gpu_shifted_windows", entry)
        qc.assert_within(entry, "shifted windows")
    finally:
        P.close()
