"""The force-fit kernel on the MI355X (pytest -m gpu): k_force_fit's table against the longdouble statement of the rule
(qtos_amd/force_fit.py, which tests/test_force_fit_cpu.py holds to first principles), its time stamps and status words, its
summary against force_fit.summarise of its own table to the bit, the accumulate flag and the ring, the host and device forms, its
argument checks, and the rings and records of ShiftedWindows.

Cases, at 1 kHz with 600 rows per window (three 256-row tiles, the last one partial), the smallest that still meet every path:
  T  the reference_compat trot, two windows: rows 0 .. 599 (four stance feet up to the phase switch at 0.3125 s, rows 312 and 313
     on its two sides, two stance feet behind it) and rows 2200 .. 2799 (three more switches)
  X  a step plan onto the ledges of exp_5, three windows with three map ids -- the ledges, flat ground, the ledges 5 mm higher --
     and three mass scales 1, 1.25, 0.8: rows 0 .. 599 (four, then three stance feet), 1500 .. 2099 and 4000 .. 4599 (the plan's
     rows with two stance feet are among them); joint rows given
  F  a 1 s schedule with a flight phase (force_fit_cases.Plan("flight")), rows 0 .. 599: rows without a stance foot; its nodes are
     a perturbed initial guess -- the fit reads nodes as data

Gates: tests/force_fit_cases.py -- per stance count and column group the larger of 8 x the float64 numpy floor measured here on
the same rows and the propagated bound K e~ with K the measured condition number of M; the device's sines and cosines are ASSUMED
good to 4 ulp, as in tests/plan_check_cases.py.  Rows within 1e-9 s of a phase switch of any foot are left out (the stance count
decides everything here): at most one row of a window at 1 kHz, and the share is held below 1 %.  The figures of the GPU run are in
profiles/force_fit_accuracy.json."""
import ctypes as C

import numpy as np
import pytest

import force_fit_cases as ffc
import plan_check_cases as pcc
from force_fit_cases import F64, LD

pytestmark = pytest.mark.gpu
HZ, N = 1000.0, 600


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Case:
    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, force_fit as ff, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name, self.maps, self.map_id, self.scale, self.cell = name, None, None, None, None
        if name == "T":
            self.cfg = PlannerConfig.reference_compat(gait="trot")
        elif name == "X":
            self.cfg = PlannerConfig.reference_compat()
        else:
            self.cfg = ffc.plan("flight").cfg
        self.P = Planner(self.cfg, max_batch=4)
        if name == "T":
            start = workloads.rest_start(0.1)[None]
            nodes, status, _, _ = self.P.plan(start, np.array([[0.1 + 0.09 * self.cfg.duration, 0.0, 0.24]]))
            assert status[0] == 0
            self.nodes, self.first = np.repeat(nodes, 2, axis=0), np.array([0, 2200], np.int32)
        elif name == "X":
            hxy, cell = workloads.exp5_terrain()
            self.maps, self.cell = np.stack([hxy, np.zeros_like(hxy), hxy + 0.005]), cell
            self.P.set_heightfields(self.maps, cell)
            start, goal = workloads.step_goals(1, seed=1, terrain=(hxy, cell))
            nodes, status, _, _ = self.P.plan(start, goal, map_id=np.zeros(1, np.int32))
            assert status[0] == 0
            self.nodes, self.map_id = np.repeat(nodes, 3, axis=0), np.array([0, 1, 2], np.int32)
            self.first, self.scale = np.array([0, 1500, 4000], np.int32), np.array([1.0, 1.25, 0.8])
        else:
            self.nodes, self.first = np.array(ffc.plan("flight").x)[None], np.array([0], np.int32)
        self.B = len(self.nodes)
        self.t0 = 3.756 + 10.0 * np.arange(self.B)
        self.L = sp.layout(self.cfg)
        self.fit = ff.fit_params(self.cfg)
        self.params = capi.fit_params(self.cfg, hz=HZ, n_rows=N, tol=ffc.TOL)
        self.joint = None
        if name == "X":
            self.joint, _ = self.P.joint_rows(self.nodes, self.t0, capi.joint_params(hz=HZ, n_rows=N), first_row=self.first)
        self.fill = -7.5
        self.rows, self.status, self.summary = self.P.force_fit(self.nodes, self.t0, self.params, map_id=self.map_id, first_row=self.first,
                                                                joint=self.joint, mass_scale=self.scale, rows=np.full((self.B, N, 32), self.fill))
        self.rows.setflags(write=False)
        self.want = {dt: [ff.fit_rows(self.L, self.nodes[b], self.t0[b], HZ, int(self.first[b]), N, self.cfg, self.fit, terrain=self.terrain(b),
                                      mass_scale=1.0 if self.scale is None else self.scale[b],
                                      joint=None if self.joint is None else self.joint[b], dtype=dt, detail=True)
                          for b in range(self.B)] for dt in (LD, F64)}
        # rows further than 1e-9 s from a phase switch of any foot
        self.decided = []
        for b in range(self.B):
            t = np.minimum((self.first[b] + np.arange(N)) / HZ, self.L.T)
            ok = np.ones(N, bool)
            for e in range(4):
                for sw in pcc.node_times(self.L.splines[2 + e])[1:-1]:
                    ok &= np.abs(t - sw) > 1e-9
            self.decided.append(ok)

    def terrain(self, b):
        return None if self.maps is None else (self.maps[self.map_id[b]], self.cell, -1.0, -1.0)

    def stance(self, b, first=None, n=N):
        from qtos_amd import plan_check as pc
        return pc.stance_rows(self.L, HZ, int(self.first[b] if first is None else first), n)


_cases = {}


def get(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(params=["T", "X", "F"])
def case(request):
    return get(request.param)


@pytest.fixture(scope="module", autouse=True)
def _close_planners():
    yield
    for c in _cases.values():
        c.P.close()
    _cases.clear()


def test_table_against_the_longdouble_statement(case):
    assert case.rows.shape == (case.B, N, 32) and N > 2 * 256
    table = case.P.sample(case.nodes, case.t0, hz=HZ, n_rows=int(case.first.max()) + N)
    counts, entry, worst = set(), {}, {}
    for b in range(case.B):
        k = case.first[b] + np.arange(N)
        assert np.array_equal(bits(case.rows[b, :, 0]), bits(table[b, k, 0]))           # qtos_sample_csv's time stamps, to the bit
        (w_ld, _, _), (w_64, _, d_64) = case.want[LD][b], case.want[F64][b]
        assert float((~case.decided[b]).mean()) <= 0.01
        groups = {g: c for g, c in ffc.GROUPS.items() if g != "tau" or case.joint is not None}
        cmp = ffc.compare(case.rows[b], w_ld, w_64, d_64, groups=groups, rows=case.decided[b])
        for c, per in cmp.items():
            counts.add(c)
            for g, w in per.items():
                key = "stance_%d_%s" % (c, g)
                if key not in worst or w["err"] / w["gate"] > worst[key]["err"] / worst[key]["gate"]:
                    worst[key] = dict(w, window=b)
        if case.joint is None:
            assert (case.rows[b, :, 20:32] == case.fill).all()                          # without joint rows the columns are not touched
        cnt = d_64["stance"].sum(axis=1)
        sw = ~d_64["stance"]
        plan_f = np.asarray(w_64[:, 1:13], F64).reshape(N, 4, 3)
        assert np.abs(case.rows[b, :, 1:13].reshape(N, 4, 3)[sw] - plan_f[sw]).max() < 1e-9   # a swing foot keeps the plan's force
    entry.update(worst)
    entry["rows_left_out"] = float(np.mean([(~d).mean() for d in case.decided]))
    ffc.record("gpu_table_" + case.name, entry)
    for key, w in worst.items():
        assert w["err"] <= w["gate"], (key, w)
    assert counts == {"T": {2, 4}, "X": {2, 3, 4}, "F": {0, 4}}[case.name]
    if case.name == "T":                                                               # rows on both sides of a phase switch
        st = case.stance(0)
        assert st[312].all() and st[313].sum() == 2
    if case.name == "X":                                                               # the three maps and mass scales are told apart
        assert case.terrain(0) is not None and np.abs(case.want[F64][2][2]["rho"][:, 5] - case.want[F64][0][2]["rho"][:, 5]).max() > 1.0


def test_status_words_equal_the_statements(case):
    from qtos_amd import force_fit as ff
    left, total, near_ld = 0, 0, 0
    for b in range(case.B):
        (w_ld, s_ld, d_ld), (_, _, d_64) = case.want[LD][b], case.want[F64][b]
        cnt = d_64["stance"].sum(axis=1)
        # rows whose excess lies within the gate of excess_tol: the bit is not decided
        near = np.zeros(N, bool)
        for c in set(int(v) for v in cnt):
            m = cnt == c
            g = ffc.gate("f_fit", 0.0, ffc.condition(d_64["M"], m) if c else 1.0) * 2.0   # (the rows of the pyramid: |(1, mu)| < 2)
            ex = np.asarray(d_ld["excess"], F64)
            near |= m & (np.abs(np.where(d_ld["stance"], ex, -np.inf) - case.fit.excess_tol) <= g).any(axis=1)
        near_ld += int(near.sum())
        keep = case.decided[b] & ~near
        left, total = left + int((~keep).sum()), total + N
        assert np.array_equal(case.status[b][keep], s_ld[keep]), (b, np.nonzero(case.status[b] != s_ld)[0][:10])
        assert not (case.status[b] & ff.NONFINITE).any()
    assert near_ld == 0 and left <= 0.01 * total, (near_ld, left, total)
    if case.name == "F":
        assert ((case.status[0] & ff.NO_STANCE) != 0).sum() >= 150


def test_summary_is_the_summary_of_the_table(case):
    from qtos_amd import capi, force_fit as ff
    for b in range(case.B):                                                            # the default call: table mode, rows count from first
        want = ff.summarise(case.rows[b], int(case.first[b]), case.stance(b), ffc.TOL, case.cfg)
        assert case.summary[b].tobytes() == want.tobytes(), (b, case.summary[b], want)
    # a ring that wraps, per-window counts with one window without rows, the rows on the windows' clocks
    B, cap = case.B, 700
    cur = np.array([123456789012 + 450 * b for b in range(B)], np.int64)               # (mod 700: 312, 62, 512: the segments wrap)
    count = np.array([N, 0, 300][:B], np.int32)
    ring = capi.fit_params(case.cfg, hz=HZ, n_rows=N, capacity=cap, tol=ffc.TOL)
    joint = None
    if case.joint is not None:
        jp = capi.joint_params(hz=HZ, n_rows=N, capacity=cap)
        joint, _ = case.P.joint_rows(case.nodes, case.t0, jp, first_row=case.first, n_rows=count, out=np.zeros((B, cap, 37)),
                                     status=np.zeros((B, cap), np.int32), cursor=cur)
    rows, status, summary = case.P.force_fit(case.nodes, case.t0, ring, map_id=case.map_id, first_row=case.first, n_rows=count, cursor=cur,
                                             joint=joint, mass_scale=case.scale, rows=np.full((B, cap, 32), case.fill),
                                             status=np.full((B, cap), -3, np.int32))
    cols = 32 if case.joint is not None else 20
    for b in range(B):
        m = int(count[b])
        at = (cur[b] + np.arange(m)) % cap
        rest = np.setdiff1d(np.arange(cap), at)
        assert (rows[b, rest] == case.fill).all() and (status[b, rest] == -3).all()    # rows behind a window's count are not touched
        assert np.array_equal(bits(rows[b, at, :cols]), bits(case.rows[b, :m, :cols])) and np.array_equal(status[b, at], case.status[b, :m])
        want = ff.summarise(case.rows[b, :m], int(cur[b]), case.stance(b, n=m), ffc.TOL, case.cfg)
        assert summary[b].tobytes() == want.tobytes(), (b, summary[b], want)
    if B > 1:
        assert summary[1].tobytes() == ff.empty_summary().tobytes() and (cur[0] % cap) + N > cap
    # QTOS_FIT_ACCUMULATE: two parts merged equal the whole, a window without rows leaves its records alone
    acc = capi.fit_params(case.cfg, hz=HZ, n_rows=250, capacity=cap, tol=ffc.TOL, accumulate=True)
    _, _, half = case.P.force_fit(case.nodes, case.t0, acc, map_id=case.map_id, first_row=case.first, cursor=cur, mass_scale=case.scale,
                                  rows=False)
    acc.n_rows = N - 250
    _, _, two = case.P.force_fit(case.nodes, case.t0, acc, map_id=case.map_id, first_row=case.first + 250, cursor=cur + 250,
                                 mass_scale=case.scale, rows=False, summary=half)
    for b in range(B):
        st = case.stance(b)
        parts = [ff.summarise(case.rows[b, :250], int(cur[b]), st[:250], ffc.TOL, case.cfg),
                 ff.summarise(case.rows[b, 250:], int(cur[b]) + 250, st[250:], ffc.TOL, case.cfg)]
        assert two[b].tobytes() == ff.accumulate(ff.accumulate(ff.empty_summary(), parts[0]), parts[1]).tobytes(), (b, two[b], parts)
        assert np.array_equal(bits(two[b]["max"]), bits(case.summary[b]["max"])) and np.array_equal(two[b]["count"], case.summary[b]["count"])
    acc.n_rows = 0
    _, _, same = case.P.force_fit(case.nodes, case.t0, acc, map_id=case.map_id, first_row=case.first, cursor=cur, rows=False, summary=two)
    assert same.tobytes() == two.tobytes()


def test_forms_equal_the_default_form_and_arguments_are_checked():
    import torch
    from qtos_amd import capi, force_fit as ff
    case = get("X")
    B = case.B
    # the host form with one output each
    rows_only, st_only, none = case.P.force_fit(case.nodes, case.t0, case.params, map_id=case.map_id, first_row=case.first, joint=case.joint,
                                                mass_scale=case.scale, summary=False)
    _, _, sum_only = case.P.force_fit(case.nodes, case.t0, case.params, map_id=case.map_id, first_row=case.first, mass_scale=case.scale,
                                      rows=False)
    assert none is None and np.array_equal(bits(rows_only), bits(case.rows)) and np.array_equal(st_only, case.status)
    assert sum_only.tobytes() == case.summary.tobytes()
    # the device form on the current stream and on a side stream
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    up = lambda a, **kw: torch.as_tensor(np.ascontiguousarray(a), device=dev, **kw)
    d_t0, d_map, d_first, d_joint, d_ms = up(case.t0), up(case.map_id), up(case.first), up(case.joint), up(case.scale)
    src = up(case.nodes)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        with torch.cuda.stream(stream):
            d_nodes = src + 0.0
            d_rows = torch.zeros((B, N, 32), **f64)
            d_st = torch.zeros((B, N), dtype=torch.int32, device=dev)
            d_sum = torch.as_tensor(ff.empty_summary(B).view(np.float64).reshape(B, 4, 3).copy(), **f64)
            case.P.force_fit(d_nodes, d_t0, case.params, map_id=d_map, first_row=d_first, joint=d_joint, mass_scale=d_ms, rows=d_rows,
                             status=d_st, summary=d_sum, stream=stream)
        stream.synchronize()
        assert np.array_equal(bits(d_rows.cpu().numpy()), bits(case.rows)) and np.array_equal(d_st.cpu().numpy(), case.status)
        assert d_sum.cpu().numpy().tobytes() == case.summary.tobytes()
    # the argument checks: -1 with the reason in qtos_last_error, nothing launched
    lib, h = case.P.lib, case.P.h
    dev_call = lambda q, rows=d_rows, st=d_st, summary=d_sum, cursor=None, nodes=src, B=B: lib.qtos_force_fit_device(
        h, B, C.byref(q), nodes.data_ptr() if nodes is not None else None, d_t0.data_ptr(), None, None, None, cursor, None, None,
        rows.data_ptr() if rows is not None else None, st.data_ptr() if st is not None else None,
        summary.data_ptr() if summary is not None else None, None)
    why = lambda: lib.qtos_last_error(h).decode()
    ok = case.params
    for kw, word in ((dict(rows=None, st=None, summary=None), "both null"), (dict(st=None), "go together"), (dict(rows=None), "go together"),
                     (dict(nodes=None), "required pointer"), (dict(B=0), "B < 1")):
        assert dev_call(ok, **kw) == -1 and word in why(), (kw, why())
    for kw, word in ((dict(arm=0.0), "arm"), (dict(damping=-1.0), "damping"), (dict(w_min=2.0), "w_min"), (dict(w_min=0.0), "w_min"),
                     (dict(excess_tol=float("nan")), "excess_tol"), (dict(l_upper=0.0), "link length"), (dict(n_rows=0), "n_rows"),
                     (dict(first_row=-1), "first_row"), (dict(first_row=1000001), "first_row"), (dict(capacity=-1), "capacity"),
                     (dict(capacity=8), "cursor")):
        q = ok.copy()
        for k, v in kw.items():
            setattr(q, k, v)
        assert dev_call(q) == -1 and word in why(), (kw, why())
    assert lib.qtos_force_fit_device(h, B, None, src.data_ptr(), d_t0.data_ptr(), None, None, None, None, None, None, d_rows.data_ptr(),
                                     d_st.data_ptr(), None, None) == -1
    torch.cuda.synchronize()
    assert dev_call(ok) == 0
    torch.cuda.synchronize()


def test_shifted_windows_fill_the_fit_ring_and_change_nothing_else():
    """B = 2, two replans behind the first plan and finish(): plans, trajectory ring and joint ring are the same bits with and
    without the fit; the fit ring equals table-mode calls over the executed segments, fit_worst() their accumulated summaries."""
    import torch
    from qtos_amd import capi, force_fit as ff, workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    B, cap, seg = 2, 700, 300
    cfg = PlannerConfig.reference_compat(gait="trot")
    start, goal = workloads.flat_goals(B, seed=7)
    P = Planner(cfg, max_batch=B)
    host = lambda t: t.cpu().numpy().copy()
    try:
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, fit=dict(tol=ffc.TOL))
        runs = {}
        for on in (False, True):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap, joints=dict(),
                               fit=dict(tol=ffc.TOL, mass_scale=[1.0, 1.1]) if on else None)
            W.replan()
            torch.cuda.synchronize()
            handed = []
            for _ in range(2):
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor), first=0, n=seg))
                W.replan()
                torch.cuda.synchronize()
                assert (host(W.row) == seg).all()
            n_all = int(round(cfg.duration * 1000.0)) + 1
            first = 0
            while first < n_all:
                n = min(n_all - first, cap)
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor) + first, first=first, n=n))
                first += n
            W.finish()
            torch.cuda.synchronize()
            if not on:
                assert W._fit is None and not hasattr(W, "fit_traj") and not hasattr(W, "fit_summary")
                with pytest.raises(RuntimeError):
                    W.fit_worst()
                with pytest.raises(RuntimeError):
                    W.fit_rows(0)
            runs[on] = dict(handed=handed, traj=host(W.traj), joint=host(W.joint_traj), jstatus=host(W.joint_status), cursor=host(W.cursor),
                            t0=host(W.t0), nodes=host(W.nodes), worst=W.fit_worst().copy() if on else None,
                            fit=[W.fit_rows(b) for b in range(B)] if on else None, jrows=[W.joint_rows(b) for b in range(B)])
        a, b = runs[False], runs[True]
        for key in ("traj", "joint", "t0", "nodes"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        assert np.array_equal(a["cursor"], b["cursor"]) and np.array_equal(a["jstatus"], b["jstatus"])
        want = ff.empty_summary(B)
        last = None
        for h in b["handed"]:
            p = capi.fit_params(cfg, hz=1000.0, first_row=h["first"], n_rows=h["n"], capacity=cap, tol=ffc.TOL)
            _, _, s = P.force_fit(h["nodes"], h["t0"], p, cursor=h["cursor"], mass_scale=[1.0, 1.1], rows=False)
            want = ff.accumulate(want, s)
            last = h
        assert b["worst"].tobytes() == want.tobytes(), (b["worst"], want)
        assert (b["worst"]["max"][:, 2] > 0.1).all() and (b["worst"]["row"] >= 0).all()
        # the ring's newest rows: the last segment in table mode, with the joint ring's rows of the same segment
        for w in range(B):
            rows, status = b["fit"][w]
            jr = b["jrows"][w][0]
            assert rows.shape == (cap, 32) and np.array_equal(bits(rows[:, 0]), bits(jr[:, 0]))
            p = capi.fit_params(cfg, hz=1000.0, first_row=last["first"], n_rows=last["n"], tol=ffc.TOL)
            t_rows, t_status, _ = P.force_fit(last["nodes"][w:w + 1], last["t0"][w:w + 1], p, mass_scale=[1.0, 1.1][w],
                                              joint=jr[None, -last["n"]:])
            assert np.array_equal(bits(rows[-last["n"]:]), bits(t_rows[0])) and np.array_equal(status[-last["n"]:], t_status[0])
        ffc.record("gpu_shifted_windows", dict(res_lin_max=[float(v) for v in b["worst"]["max"][:, 1]],
                                               change_max=[float(v) for v in b["worst"]["max"][:, 2]]))
    finally:
        P.close()


def test_c_caller_prints_the_same_summary(tmp_path):
    import os
    import re
    import subprocess
    from conftest import ROOT
    from qtos_amd import capi
    case = get("T")
    csrc = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
    exe = tmp_path / "forcefit_caller"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "forcefit_caller.c"), "-o", str(exe), "-L", csrc, "-lqtos_planner",
                           "-Wl,-rpath," + csrc, "-Wl,--allow-shlib-undefined"])
    img, out = tmp_path / "params.bin", tmp_path / "nodes.bin"
    img.write_bytes(bytes(capi.params_from_config(case.cfg)))
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), str(img), str(out)], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "bad_args=-1,-1,-1,-1,-1,-1,-1,-1" in r.stdout and "stamp_mismatches=0 differ=0" in r.stdout
    assert int(re.search(r"two_stance_rows=(\d+)", r.stdout).group(1)) > 800
    # the caller's two plans, its clocks and its parameters through the Python form
    nodes = np.fromfile(str(out), np.float64).reshape(2, case.P.n)
    _, _, summary = case.P.force_fit(nodes, np.array([0.0, 10.0]), capi.fit_params(case.cfg, hz=100.0, n_rows=520), rows=False)
    got = re.findall(r"window (\d) (\w+) max=\S+ bits=([0-9a-f]+) row=(-?\d+) count=(\d+)", r.stdout)
    assert len(got) == 8
    for b, fam, mx, row, count in got:
        s = summary[int(b)][["res_ang", "res_lin", "change", "excess"].index(fam)]
        assert (int(mx, 16), int(row), int(count)) == (int(bits(s["max"]).reshape(-1)[0]), int(s["row"]), int(s["count"])), (b, fam, s)


def test_solve_and_command_line_print_the_fit(tmp_path):
    """LocalPlanner.solve(fit=...) writes one line per family behind the solve and keeps the records; `python -m qtos_amd.main ...
    --fit` prints the same lines in front of the status line; CSV and exit status are what they are without it."""
    import io
    import os
    import subprocess
    import sys
    from conftest import ROOT, load_gv
    from oracle import splines as sp
    from qtos_amd import capi, flags, force_fit as ff, plan_check as pc
    from qtos_amd.planner import LocalPlanner
    inp = load_gv("gv1")["inputs"]
    args = {"-g": inp["g"], "-s": inp["s"], "-s_ang": [0, 0, 0], "-e1": inp["ee"][0], "-e2": inp["ee"][1],
            "-e3": inp["ee"][2], "-e4": inp["ee"][3], "-t": 3.756, "-resolution": 0.01, "scripts": {}}
    lp = LocalPlanner(max_batch=1)
    try:
        buf = io.StringIO()
        assert lp.solve(args, out_csv=str(tmp_path / "a.csv"), fit=buf) == 0
        lines = buf.getvalue().splitlines()
        summary = lp.last["fit"]
        assert len(lines) == 4 and [ln.split()[2] for ln in lines] == list(ff.FAMILIES)
        assert lines == ff.report_lines(summary, 3.756, 1000.0, capi.FIT_TOL)
        rows, _, want = lp.planner().force_fit(lp.last["nodes"][:1], 3.756, capi.fit_params(lp.cfg, n_rows=5001))
        stance = pc.stance_rows(sp.layout(lp.cfg), 1000.0, 0, 5001)
        assert summary.tobytes() == want[0].tobytes() == ff.summarise(rows[0], 0, stance, capi.FIT_TOL, lp.cfg).tobytes()
        assert 0.1 < summary["max"][2] < 10.0 and summary["max"][1] < 1.0             # newtons moved, what is left on two-stance rows
        assert lp.solve(args, out_csv=str(tmp_path / "b.csv")) == 0 and "fit" not in lp.last
    finally:
        lp.close()
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "qtos_amd.main"] + flags.cmd_args(args).split() + ["--out", str(tmp_path / "c.csv"), "--fit"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert out[-1] == "status -> 0" and out[-5:-1] == lines
    assert open(tmp_path / "c.csv", "rb").read() == open(tmp_path / "a.csv", "rb").read()
