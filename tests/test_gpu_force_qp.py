"""The force-QP kernel on the MI355X (pytest -m gpu): k_force_qp's two tables against the longdouble statement of the rule
(qtos_amd/force_qp.py, which tests/test_force_qp_cpu.py holds to a certificate and to the optimum by enumeration), its status
words, its summary against force_qp.summarise of its own tables to the bit, the shapes at the edges of a tile, the ring, the host
and device forms and the argument checks.

Cases and gates: tests/force_qp_cases.py -- 251 rows per plan at 50 Hz (two tiles of 128 lanes, the second partial), 69 rows of
the synthetic ones.  A gate is 8 x the float64 numpy floor of the group over the rows of all cases (force_qp_cases.group_floors); the device's sines and cosines are
ASSUMED good to 4 ulp, as in tests/plan_check_cases.py.  Rows whose fit's largest limit-row value lies within the guard band
of 0 are left out (the path switch is a discontinuity there), and for the status words also rows with a slack within the
slack group's gate of act_tol (the bit is not decided); their share is held below 1 %.  Step counts may differ from the rule's
by one where the last step's complementarity lies at CTOL.  Columns 1 and 2 of the solve's table are held to the thresholds the
iteration stops at.  The figures of the GPU run are in profiles/force_qp_accuracy.json."""
import ctypes as C

import numpy as np
import pytest

import force_qp_cases as qc
from force_qp_cases import F64, LD

pytestmark = pytest.mark.gpu
TILE = 128


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Gpu:
    """A case on the device: its planner (one per configuration), the kernel's tables of the case's rows."""
    planners = {}

    def __init__(self, name):
        from qtos_amd import capi
        from qtos_amd.capi import Planner
        c = self.c = qc.case(name)
        key = "ledge" if name == "ledge" else ("trot" if "trot" in name else "walk")
        if key not in Gpu.planners:
            P = Planner(c.cfg, max_batch=4)
            if key == "ledge":
                P.set_heightfields(c.terrain[0][None], c.terrain[1])
            Gpu.planners[key] = P
        self.P = Gpu.planners[key]
        self.nodes, self.t0 = np.array(c.x)[None], np.array([qc.T0])
        kw = dict(mu=c.qp.mu, f_max=c.qp.f_max, mu_end=c.qp.mu_end, act_tol=c.qp.act_tol, max_iter=c.qp.max_iter)
        self.kw = kw
        self.params = capi.qp_params(c.cfg, hz=c.hz, first_row=c.first, n_rows=c.n, tol=qc.TOL, **kw)
        self.map_id = np.zeros(1, np.int32) if key == "ledge" else None
        self.joint = None
        if name == "ledge":
            self.joint, _ = self.P.joint_rows(self.nodes, self.t0, capi.joint_params(hz=c.hz, first_row=c.first, n_rows=c.n))
        self.fill = -7.5
        self.rows, self.qrows, self.status, self.summary = self.P.force_qp(
            self.nodes, self.t0, self.params, map_id=self.map_id, joint=self.joint, rows=np.full((1, c.n, 32), self.fill))
        for a in (self.rows, self.qrows, self.status):
            a.setflags(write=False)

    def want(self, dtype):
        return self.c.rows(dtype, None if self.joint is None else self.joint[0])


_gpu = {}


def get(name):
    if name not in _gpu:
        _gpu[name] = Gpu(name)
    return _gpu[name]


@pytest.fixture(params=qc.NAMES)
def case(request):
    return get(request.param)


@pytest.fixture(scope="module", autouse=True)
def _close_planners():
    yield
    for P in Gpu.planners.values():
        P.close()
    Gpu.planners.clear()
    _gpu.clear()


def test_tables_against_the_longdouble_statement(case):
    from qtos_amd import force_qp as fq
    c = case.c
    old, qld, sld, Dld = case.want(LD)
    joint = None if case.joint is None else case.joint[0]
    band, inb = qc.guard(c)
    assert inb.mean() <= 0.01
    keep = ~inb
    fl = qc.group_floors(get("ledge").joint[0])
    table = case.P.sample(case.nodes, case.t0, hz=c.hz, n_rows=c.first + c.n)
    assert np.array_equal(bits(case.rows[0, :, 0]), bits(table[0, c.first:c.first + c.n, 0]))      # qtos_sample_csv's time stamps, to the bit
    entry = {}
    for g, sl in list(qc.GROUPS.items()) + list(qc.QGROUPS.items()):
        if g == "tau" and joint is None:
            continue
        got = case.qrows[0] if g in qc.QGROUPS else case.rows[0]
        ref = qld if g in qc.QGROUPS else old
        entry[g] = dict(err=qc.dist(got[keep][:, sl], ref[keep][:, sl]), floor=fl[g], gate=qc.MARGIN * fl[g])
    lim = Dld["limited"] & keep
    q = case.qrows[0]
    entry["comp"] = dict(err=float(q[lim, 1].max()), gate=fq.CTOL)
    entry["steps_differ"] = int((q[keep, 0] != np.asarray(qld[keep, 0], F64)).sum())
    entry["steps_max"], entry["rows"], entry["limited_rows"], entry["in_band"] = int(q[:, 0].max()), c.n, int(lim.sum()), int(inb.sum())
    qc.record("gpu_tables_" + c.name, entry)
    if joint is None:
        assert (case.rows[0, :, 20:32] == case.fill).all()                                         # without joint rows the columns are not touched
    sw = ~Dld["stance"]
    assert np.abs(case.rows[0, :, 1:13].reshape(-1, 4, 3)[sw] - np.asarray(Dld["f"], F64)[sw]).max() < 1e-9   # a swing foot keeps the plan's force
    assert np.abs(q[keep, 0] - np.asarray(qld[keep, 0], F64)).max() <= 1
    cap = (case.status[0] & fq.CAP) != 0
    assert not cap.any()
    assert (q[lim, 1] <= fq.CTOL).all() and (q[lim, 2] <= fq.RTOL * (1 + 50.0)).all()             # (|q|inf: forces of the order of 20 N)
    assert (q[lim, 3] > 0).all() and (q[lim, 6] >= 0).all()
    for g, w in entry.items():
        if isinstance(w, dict) and "floor" in w:
            assert w["err"] <= w["gate"], (g, w)


def test_status_words_equal_the_statements(case):
    from qtos_amd import force_qp as fq
    c = case.c
    _, qld, sld, Dld = case.want(LD)
    band, inb = qc.guard(c)
    fl = qc.group_floors(get("ledge").joint[0])
    near = (np.abs(np.where(Dld["stance"][:, :, None], np.asarray(Dld["slack"], F64), np.inf) - c.qp.act_tol) <= qc.MARGIN * fl["slack"]).any(axis=(1, 2))
    keep = ~inb & ~near
    assert (~keep).mean() <= 0.01, (int(inb.sum()), int(near.sum()))
    assert np.array_equal(case.status[0][keep], sld[keep]), np.nonzero(case.status[0] != sld)[0][:10]
    assert np.array_equal(case.qrows[0][keep, 7], np.asarray(qld[keep, 7], F64))
    assert not (case.status[0] & fq.NONFINITE).any() and ((case.status[0] & fq.LIMITED) != 0).mean() >= 0.05


def test_summary_is_the_summary_of_the_tables(case):
    from qtos_amd import capi, force_qp as fq
    c = case.c
    want = fq.summarise(case.rows[0], case.qrows[0], c.first, qc.TOL)
    assert case.summary[0].tobytes() == want.tobytes(), (case.summary[0], want)
    # a ring that wraps, the rows on the window's clock, and the accumulate flag: two parts merged equal the whole
    cap = c.n + 37
    cur = np.array([428600000 * cap + cap - 20], np.int64)                           # the segment wraps after 20 rows
    assert (cur[0] % cap) + c.n > cap
    ring = capi.qp_params(c.cfg, hz=c.hz, first_row=c.first, n_rows=c.n, capacity=cap, tol=qc.TOL, **case.kw)
    joint = None
    if case.joint is not None:
        jp = capi.joint_params(hz=c.hz, first_row=c.first, n_rows=c.n, capacity=cap)
        joint, _ = case.P.joint_rows(case.nodes, case.t0, jp, out=np.zeros((1, cap, 37)), status=np.zeros((1, cap), np.int32), cursor=cur)
    rows, qrows, status, summary = case.P.force_qp(case.nodes, case.t0, ring, map_id=case.map_id, cursor=cur, joint=joint,
                                                   rows=np.full((1, cap, 32), case.fill), qrows=np.full((1, cap, 8), case.fill),
                                                   status=np.full((1, cap), -3, np.int32))
    at = (cur[0] + np.arange(c.n)) % cap
    rest = np.setdiff1d(np.arange(cap), at)
    cols = 32 if joint is not None else 20
    assert (rows[0, rest] == case.fill).all() and (qrows[0, rest] == case.fill).all() and (status[0, rest] == -3).all()
    assert np.array_equal(bits(rows[0, at, :cols]), bits(case.rows[0, :, :cols])) and np.array_equal(bits(qrows[0, at]), bits(case.qrows[0]))
    assert np.array_equal(status[0, at], case.status[0])
    assert summary[0].tobytes() == fq.summarise(case.rows[0], case.qrows[0], int(cur[0]), qc.TOL).tobytes()
    half = c.n // 2
    acc = capi.qp_params(c.cfg, hz=c.hz, first_row=c.first, n_rows=half, capacity=cap, tol=qc.TOL, accumulate=True, **case.kw)
    _, _, _, one = case.P.force_qp(case.nodes, case.t0, acc, map_id=case.map_id, cursor=cur, rows=False)
    acc.first_row, acc.n_rows = c.first + half, c.n - half
    _, _, _, two = case.P.force_qp(case.nodes, case.t0, acc, map_id=case.map_id, cursor=cur + half, rows=False, summary=one)
    parts = [fq.summarise(case.rows[0, :half], case.qrows[0, :half], int(cur[0]), qc.TOL),
             fq.summarise(case.rows[0, half:], case.qrows[0, half:], int(cur[0]) + half, qc.TOL)]
    assert two[0].tobytes() == fq.accumulate(fq.accumulate(fq.empty_summary(), parts[0]), parts[1]).tobytes(), (two[0], parts)


def test_shapes_forms_and_argument_checks():
    import torch
    from qtos_amd import capi, force_qp as fq
    case = get("trot")
    c = case.c
    assert c.n > TILE + 1
    for n in (1, TILE - 1, TILE, TILE + 1):
        p = capi.qp_params(c.cfg, hz=c.hz, first_row=c.first, n_rows=n, tol=qc.TOL, **case.kw)
        rows, qrows, status, summary = case.P.force_qp(case.nodes, case.t0, p)
        assert np.array_equal(bits(rows[0, :, :20]), bits(case.rows[0, :n, :20])) and np.array_equal(bits(qrows[0]), bits(case.qrows[0, :n]))
        assert np.array_equal(status[0], case.status[0, :n])
        assert summary[0].tobytes() == fq.summarise(rows[0], qrows[0], c.first, qc.TOL).tobytes()
    # summary only; rows without qrows; rows without a summary
    _, none_q, none_s, sum_only = case.P.force_qp(case.nodes, case.t0, case.params, rows=False)
    assert none_q is None and none_s is None and sum_only.tobytes() == case.summary.tobytes()
    rows, no_q, status, no_sum = case.P.force_qp(case.nodes, case.t0, case.params, qrows=False, summary=False)
    assert no_q is None and no_sum is None and np.array_equal(bits(rows[0, :, :20]), bits(case.rows[0, :, :20])) and np.array_equal(status, case.status)
    # the device form on the current stream and on a side stream equals the host form to the bit
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a, **kw: torch.as_tensor(np.ascontiguousarray(a), device=dev, **kw)
    d_t0, src = up(case.t0), up(case.nodes)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        with torch.cuda.stream(stream):
            d_nodes = src + 0.0
            d_rows, d_q = torch.zeros((1, c.n, 32), **f64), torch.zeros((1, c.n, 8), **f64)
            d_st = torch.zeros((1, c.n), dtype=torch.int32, device=dev)
            d_sum = torch.as_tensor(fq.empty_summary(1).view(np.float64).reshape(1, 4, 3).copy(), **f64)
            case.P.force_qp(d_nodes, d_t0, case.params, rows=d_rows, qrows=d_q, status=d_st, summary=d_sum, stream=stream)
        stream.synchronize()
        assert np.array_equal(bits(d_rows.cpu().numpy()[0, :, :20]), bits(case.rows[0, :, :20])) and np.array_equal(bits(d_q.cpu().numpy()), bits(case.qrows))
        assert np.array_equal(d_st.cpu().numpy(), case.status) and d_sum.cpu().numpy().tobytes() == case.summary.tobytes()
    # the argument checks: -1 with the reason in qtos_last_error, nothing launched
    lib, h = case.P.lib, case.P.h
    dev_call = lambda q, rows=d_rows, qr=d_q, st=d_st, summary=d_sum, cursor=None, nodes=src, B=1: lib.qtos_force_qp_device(
        h, B, C.byref(q), nodes.data_ptr() if nodes is not None else None, d_t0.data_ptr(), None, None, None, cursor, None, None,
        rows.data_ptr() if rows is not None else None, qr.data_ptr() if qr is not None else None, st.data_ptr() if st is not None else None,
        summary.data_ptr() if summary is not None else None, None)
    why = lambda: lib.qtos_last_error(h).decode()
    ok = case.params
    for kw, word in ((dict(rows=None, qr=None, st=None, summary=None), "both null"), (dict(st=None), "go together"), (dict(rows=None, qr=None), "go together"),
                     (dict(rows=None, st=None), "qrows go with rows"), (dict(nodes=None), "required pointer"), (dict(B=0), "B < 1")):
        assert dev_call(ok, **kw) == -1 and word in why() and why().startswith("qtos_force_qp"), (kw, why())
    for kw, word in ((dict(mu=0.0), "mu is"), (dict(mu=float("nan")), "mu is"), (dict(f_max=0.0), "f_max"), (dict(f_max=-1.0), "f_max"),
                     (dict(mu_end=0.0), "mu_end"), (dict(act_tol=float("nan")), "act_tol"), (dict(max_iter=0), "max_iter"), (dict(max_iter=26), "max_iter"),
                     (dict(arm=0.0), "arm"), (dict(damping=-1.0), "damping"), (dict(w_min=2.0), "w_min"), (dict(l_upper=0.0), "link length"),
                     (dict(n_rows=0), "n_rows"), (dict(first_row=-1), "first_row"), (dict(capacity=-1), "capacity"), (dict(capacity=8), "cursor")):
        q = ok.copy()
        for k, v in kw.items():
            setattr(q, k, v)
        assert dev_call(q) == -1 and word in why(), (kw, why())
    assert lib.qtos_force_qp_device(h, 1, None, src.data_ptr(), d_t0.data_ptr(), None, None, None, None, None, None, d_rows.data_ptr(), d_q.data_ptr(),
                                    d_st.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert dev_call(ok) == 0
    torch.cuda.synchronize()


def test_shifted_windows_fill_both_rings_and_change_nothing_else():
    """B = 2, two replans behind the first plan and finish(): plans, trajectory ring and joint ring are the same bits without a fit,
    with the fit and with the fit inside its limits; with limits= the fit ring and the ring of the solve's table equal table-mode
    calls over the executed segments, fit_worst() their accumulated summaries."""
    import torch
    from qtos_amd import capi, force_qp as fq, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    B, cap, seg = 2, 700, 300
    lim = dict(f_max=16.0, mu=0.4)
    cfg = PlannerConfig.reference_compat(gait="trot")
    start, goal = workloads.flat_goals(B, seed=7)
    P = Planner(cfg, max_batch=B)
    host = lambda t: t.cpu().numpy().copy()
    try:
        runs = {}
        for mode in ("none", "fit", "limits"):
            fit = None if mode == "none" else dict(tol=qc.TOL, mass_scale=[1.0, 1.1], **(dict(limits=lim) if mode == "limits" else {}))
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(), fit=fit)
            W.replan()
            torch.cuda.synchronize()
            handed = []
            for _ in range(2):
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor), first=0, n=seg))
                W.replan()
                torch.cuda.synchronize()
            n_all = int(round(cfg.duration * 1000.0)) + 1
            first = 0
            while first < n_all:
                n = min(n_all - first, cap)
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor) + first, first=first, n=n))
                first += n
            W.finish()
            torch.cuda.synchronize()
            if mode != "limits":
                assert not hasattr(W, "qp_traj")
                with pytest.raises(RuntimeError):
                    W.qp_rows(0)
            runs[mode] = dict(handed=handed, traj=host(W.traj), joint=host(W.joint_traj), jstatus=host(W.joint_status), cursor=host(W.cursor),
                              t0=host(W.t0), nodes=host(W.nodes), worst=None if mode == "none" else W.fit_worst().copy(),
                              fit=None if mode == "none" else [W.fit_rows(b) for b in range(B)],
                              qp=[W.qp_rows(b) for b in range(B)] if mode == "limits" else None, jrows=[W.joint_rows(b) for b in range(B)])
        a = runs["none"]
        for mode in ("fit", "limits"):
            for key in ("traj", "joint", "t0", "nodes"):
                assert np.array_equal(bits(a[key]), bits(runs[mode][key])), (mode, key)
            assert np.array_equal(a["cursor"], runs[mode]["cursor"]) and np.array_equal(a["jstatus"], runs[mode]["jstatus"])
        b = runs["limits"]
        want, last = fq.empty_summary(B), None
        for h in b["handed"]:
            p = capi.qp_params(cfg, hz=1000.0, first_row=h["first"], n_rows=h["n"], capacity=cap, tol=qc.TOL, **lim)
            _, _, _, s = P.force_qp(h["nodes"], h["t0"], p, cursor=h["cursor"], mass_scale=[1.0, 1.1], rows=False)
            want, last = fq.accumulate(want, s), h
        assert b["worst"].tobytes() == want.tobytes(), (b["worst"], want)
        assert (b["worst"]["max"][:, 3] > 0.1).all()                                              # the cap moved forces
        for w in range(B):
            rows, status = b["fit"][w]
            jr = b["jrows"][w][0]
            assert rows.shape == (cap, 32) and b["qp"][w].shape == (cap, 8) and np.array_equal(bits(rows[:, 0]), bits(jr[:, 0]))
            p = capi.qp_params(cfg, hz=1000.0, first_row=last["first"], n_rows=last["n"], tol=qc.TOL, **lim)
            t_rows, t_q, t_status, _ = P.force_qp(last["nodes"][w:w + 1], last["t0"][w:w + 1], p, mass_scale=[1.0, 1.1][w], joint=jr[None, -last["n"]:])
            assert np.array_equal(bits(rows[-last["n"]:]), bits(t_rows[0])) and np.array_equal(status[-last["n"]:], t_status[0])
            assert np.array_equal(bits(b["qp"][w][-last["n"]:]), bits(t_q[0]))
            # the fit path's rows of the limits run against the plain fit's: the same forces where nothing was limited
            free = (status & fq.LIMITED) == 0
            assert free.any() and np.abs(rows[free, 1:13] - runs["fit"]["fit"][w][0][free, 1:13]).max() < 1e-6
    finally:
        P.close()
