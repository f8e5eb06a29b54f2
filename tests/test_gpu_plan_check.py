"""The plan-check kernel on the MI355X (pytest -m gpu): k_plan_check's table against the longdouble statement of the rule
(qtos_amd/plan_check.py, which tests/test_plan_check_cpu.py holds to the C oracle), its summary against plan_check.summarise of
its own table to the bit, the accumulate flag, a NaN node, a non-default stream, the host form, either output alone, the call
from plain C and the records of ShiftedWindows.

Cases, the smallest that can still go wrong:
  S  PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5) at 500 Hz, 600 rows: three 256-row tiles,
     the last one partial; rows 501 .. 599 lie past the horizon and are clamped to it
  T  the reference_compat trot at 100 Hz, 520 rows
  X  a step plan onto the ledges of exp_5, three windows with three different map ids: the ledges, flat ground, the ledges 5 mm
     higher -- a kernel that reads another window's map fails it

Gates: tests/plan_check_cases.py -- per column group the larger of 8 x the float64 numpy floor measured here and the propagated
bound, capped at 1e-10; the device's sines and cosines are ASSUMED good to 4 ulp.  Columns 23 .. 26 depend on whether the foot's
polynomial is a stance or a swing: they are compared on rows further than 1e-9 s from a phase switch of any foot, and the share
of rows left out is reported and held below 1 % (S and X: none, T: 3 of 520).  Measured on an MI355X
(profiles/plan_check_accuracy.json), the worst of the three cases against the longdouble statement: dynamics 1.2e-12 N / 3.3e-14
N m, range of motion 9.5e-15 m, clearance 9.5e-15 m, force 2.4e-13 N, each equal to the float64 numpy floor to two digits."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plan_check_cases as pcc
from conftest import ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LD, F64 = np.longdouble, np.float64


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Case:
    def __init__(self, name):
        from oracle import splines as sp
        from qtos_amd import capi, plan_check as pc, workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.name, self.maps, self.map_id = name, None, None
        if name == "S":
            self.cfg = PlannerConfig(duration=1.0, dt_base=0.5, dt_dynamic=0.5, dt_range_of_motion=0.5)
            self.hz, self.n = 500.0, 600
        elif name == "T":
            self.cfg = PlannerConfig.reference_compat(gait="trot")
            self.hz, self.n = 100.0, 520
        else:
            self.cfg = PlannerConfig.reference_compat()
            self.hz, self.n = 100.0, 520
        self.P = Planner(self.cfg, max_batch=4)
        if name == "X":
            hxy, cell = workloads.exp5_terrain()
            self.maps, self.cell = np.stack([hxy, np.zeros_like(hxy), hxy + 0.005]), cell
            self.P.set_heightfields(self.maps, cell)
            start, goal = workloads.step_goals(1, seed=1, terrain=(hxy, cell))
            nodes, status, _, _ = self.P.plan(start, goal, map_id=np.zeros(1, np.int32))
            self.nodes, self.map_id = np.repeat(nodes, 3, axis=0), np.array([0, 1, 2], np.int32)
        else:
            start = workloads.rest_start(0.1)[None]
            goal = np.array([[0.1 + 0.09 * self.cfg.duration, 0.0, 0.24]])
            self.nodes, status, _, _ = self.P.plan(start, goal)
        assert status[0] == 0
        self.B = len(self.nodes)
        self.t0 = 3.756 + 10.0 * np.arange(self.B)
        self.L = sp.layout(self.cfg)
        self.params = capi.check_params(hz=self.hz, n_rows=self.n, tol=pcc.TOL)
        self.rows, self.summary = self.P.plan_check(self.nodes, self.t0, self.params, map_id=self.map_id)
        self.rows.setflags(write=False)
        self.stance = pc.stance_rows(self.L, self.hz, 0, self.n)
        self.want = {}
        for dt in (LD, F64):
            self.want[dt] = [pc.check_rows(self.L, self.nodes[b], self.t0[b], self.hz, 0, self.n, self.cfg, terrain=self.terrain(b), dtype=dt)
                             for b in range(self.B)]
        # rows further than 1e-9 s from a phase switch of any foot
        t = np.minimum(np.arange(self.n) / self.hz, self.L.T)
        self.decided = np.ones(self.n, bool)
        for e in range(4):
            for sw in pcc.node_times(self.L.splines[2 + e])[1:-1]:
                self.decided &= np.abs(t - sw) > 1e-9

    def terrain(self, b):
        return None if self.maps is None else (self.maps[self.map_id[b]], self.cell, -1.0, -1.0)


_cases = {}


def get(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


@pytest.fixture(params=["S", "T", "X"])
def case(request):
    return get(request.param)


@pytest.fixture(scope="module", autouse=True)
def _close_planners():
    yield
    for c in _cases.values():
        c.P.close()
    _cases.clear()


def test_table_against_the_longdouble_statement(case):
    table = case.P.sample(case.nodes, case.t0, hz=case.hz, n_rows=case.n)
    assert case.rows.shape == (case.B, case.n, 27)
    assert np.array_equal(bits(case.rows[:, :, 0]), bits(table[:, :, 0]))              # qtos_sample_csv's time stamps, to the bit
    left_out = float((~case.decided).mean())
    entry = dict(rows_left_out=left_out)
    assert left_out <= 0.01
    if case.name == "S":
        assert case.n > 2 * 256 and (case.n - 1) / case.hz > case.L.T                  # a partial third tile, rows past the horizon
        tail = case.rows[0, int(case.L.T * case.hz) + 1:, 1:]
        assert np.array_equal(bits(tail), bits(np.broadcast_to(tail[0], tail.shape)))  # behind the horizon the plan's last row
    worst = {}
    for b in range(case.B):
        w_ld, w_64 = case.want[LD][b], case.want[F64][b]
        for group, cols in pcc.GROUPS.items():
            rows = case.decided if group == "force" else np.ones(case.n, bool)
            floor = float(np.abs(w_64[rows, cols].astype(LD) - w_ld[rows, cols]).max())
            err = float(np.abs(case.rows[b][rows, cols].astype(LD) - w_ld[rows, cols]).max())
            g = pcc.gate(group, floor)
            if group not in worst or err / g > worst[group]["err"] / worst[group]["gate"]:
                worst[group] = dict(err=err, floor=floor, gate=g, window=b)
    entry.update(worst)
    pcc.record("gpu_table_" + case.name, entry)
    for group, w in worst.items():
        assert w["err"] <= w["gate"], (group, w)
    if case.name == "X":                                                               # the three maps are told apart
        c = case.rows[:, :, 19:23]
        assert np.abs(c[0] - c[1]).max() > 0.02 and np.abs(c[2] - c[0] + 0.005).max() < 1e-12


def test_summary_is_the_summary_of_the_table(case):
    from qtos_amd import plan_check as pc
    for b in range(case.B):                                                            # the default call: every row of every window
        want = pc.summarise(case.rows[b], 0, case.stance, pcc.TOL)
        assert case.summary[b].tobytes() == want.tobytes(), (b, case.summary[b], want)
    # per-window first rows and counts, one window without rows
    B = 3
    nodes, t0 = np.repeat(case.nodes[:1], B, axis=0), case.t0[0] + np.arange(B)
    mid = None if case.map_id is None else np.array([2, 0, 1], np.int32)
    first, count = np.array([0, 7, 100], np.int32), np.array([case.n, 0, 300], np.int32)
    fill = np.full((B, case.n, 27), -7.5)
    rows, summary = case.P.plan_check(nodes, t0, case.params, map_id=mid, first_row=first, n_rows=count, rows=fill)
    for b in range(B):
        m = int(count[b])
        assert (rows[b, m:] == -7.5).all()                                             # rows behind a window's count are not touched
        stance = pc.stance_rows(case.L, case.hz, int(first[b]), m)
        want = pc.summarise(rows[b, :m], int(first[b]), stance, pcc.TOL)
        assert summary[b].tobytes() == want.tobytes(), (b, summary[b], want)
        if m and mid is None:                                                          # the rows are the table's rows first .. first + m - 1
            k = first[b] + np.arange(m)
            assert np.array_equal(bits(rows[b, :m, 1:]), bits(case.rows[0][k, 1:]))
    assert summary[1].tobytes() == pc.empty_summary().tobytes()
    assert (case.summary["max"][:, :2] > 0).all() and (case.summary["row"] >= 0).all()


def test_accumulate_two_halves_equal_the_whole():
    from qtos_amd import capi, plan_check as pc
    case = get("S")
    cur = np.array([123456789012], np.int64)
    whole = capi.check_params(hz=case.hz, n_rows=600, tol=pcc.TOL)
    _, one = case.P.plan_check(case.nodes, case.t0, whole, cursor=cur, rows=False)
    assert (one["row"] >= cur[0]).all() and np.array_equal(one["row"] - cur[0], case.summary["row"])
    assert np.array_equal(bits(one["max"]), bits(case.summary["max"])) and np.array_equal(one["count"], case.summary["count"])
    acc = capi.check_params(hz=case.hz, first_row=0, n_rows=300, tol=pcc.TOL, accumulate=True)
    _, half = case.P.plan_check(case.nodes, case.t0, acc, cursor=cur, rows=False)
    acc.first_row = 300
    _, two = case.P.plan_check(case.nodes, case.t0, acc, cursor=cur + 300, rows=False, summary=half)
    assert two.tobytes() == one.tobytes(), (two, one)
    # the numpy accumulate of the two halves of the kernel's own table is the same
    st = case.stance
    parts = [pc.summarise(case.rows[0, :300], cur[0], st[:300], pcc.TOL), pc.summarise(case.rows[0, 300:], cur[0] + 300, st[300:], pcc.TOL)]
    assert pc.accumulate(pc.accumulate(pc.empty_summary(), parts[0]), parts[1]).tobytes() == one[0].tobytes()
    # without the flag the record is overwritten
    plain = capi.check_params(hz=case.hz, first_row=300, n_rows=300, tol=pcc.TOL)
    _, over = case.P.plan_check(case.nodes, case.t0, plain, cursor=cur + 300, rows=False, summary=half)
    assert over[0].tobytes() == parts[1].tobytes()


def test_nan_node_in_one_window():
    from qtos_amd import plan_check as pc
    case = get("T")
    B = 3
    nodes, t0 = np.repeat(case.nodes[:1], B, axis=0), np.repeat(case.t0[:1], B)
    sp = case.L.splines
    nodes[1, np.asarray(sp[0].idx).reshape(-1, 2, 3)[20, 0, 0]] = np.nan              # the base's x at node 20: rows 190 .. 210
    nodes[1, np.asarray(sp[2].idx).reshape(-1, 2, 3)[4, 0, 1]] = np.nan               # the y of a later foothold of foot 0
    rows, summary = case.P.plan_check(nodes, t0, case.params)
    for b in (0, 2):
        assert np.array_equal(bits(rows[b]), bits(case.rows[0])) and summary[b].tobytes() == case.summary[0].tobytes()
    want = pc.summarise(pc.check_rows(case.L, nodes[1], t0[1], case.hz, 0, case.n, case.cfg), 0, case.stance, pcc.TOL)
    assert (want["max"] == np.inf).all()                                               # the statement: every family is hit
    assert (summary[1]["max"] == np.inf).all() and np.array_equal(summary[1]["row"], want["row"]), (summary[1], want)
    assert np.array_equal(summary[1]["count"], want["count"])
    assert summary[1].tobytes() == pc.summarise(rows[1], 0, case.stance, pcc.TOL).tobytes()


def test_forms_equal_the_default_form():
    import torch
    from qtos_amd import plan_check as pc
    case = get("X")
    B = case.B
    # the host form with one output each
    rows_only, none = case.P.plan_check(case.nodes, case.t0, case.params, map_id=case.map_id, summary=False)
    none2, sum_only = case.P.plan_check(case.nodes, case.t0, case.params, map_id=case.map_id, rows=False)
    assert none is None and none2 is None
    assert np.array_equal(bits(rows_only), bits(case.rows)) and sum_only.tobytes() == case.summary.tobytes()
    # the device form on the current stream and on a side stream that has to wait for nothing of ours
    dev = torch.device("cuda", 0)
    f64 = dict(dtype=torch.float64, device=dev)
    d_t0, d_map = torch.as_tensor(case.t0, **f64), torch.as_tensor(case.map_id, device=dev)
    src = torch.as_tensor(case.nodes, **f64)
    side = torch.cuda.Stream(dev)
    torch.cuda.synchronize()
    for stream in (torch.cuda.current_stream(dev), side):
        with torch.cuda.stream(stream):
            d_nodes = src + 0.0
            d_rows = torch.zeros((B, case.n, 27), **f64)
            d_sum = torch.as_tensor(pc.empty_summary(B).view(np.float64).reshape(B, 5, 3).copy(), **f64)
            case.P.plan_check(d_nodes, d_t0, case.params, map_id=d_map, rows=d_rows, summary=d_sum, stream=stream)
        stream.synchronize()
        assert np.array_equal(bits(d_rows.cpu().numpy()), bits(case.rows))
        assert d_sum.cpu().numpy().tobytes() == case.summary.tobytes()
    # both outputs NULL: -1
    rc = case.P.lib.qtos_plan_check_device(case.P.h, B, C.byref(case.params), src.data_ptr(), d_t0.data_ptr(), None, None, None, None,
                                           None, None, None)
    assert rc == -1


def test_c_caller_prints_the_same_summary(tmp_path):
    from qtos_amd import capi
    case = get("T")
    exe = tmp_path / "plancheck_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "plancheck_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    subprocess.check_call(cmd)
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(case.cfg)))
    out = tmp_path / "nodes.bin"
    r = subprocess.run([str(exe), str(img), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "bad_args=-1,-1,-1,-1,-1,-1" in r.stdout and "stamp_mismatches=0" in r.stdout and "differ=0" in r.stdout
    # the caller's two plans, its clocks and its parameters through the Python form
    nodes = np.fromfile(str(out), np.float64).reshape(2, case.P.n)
    _, summary = case.P.plan_check(nodes, np.array([0.0, 10.0]), capi.check_params(hz=100.0, n_rows=520), rows=False)
    got = re.findall(r"window (\d) (\w+) max=\S+ bits=([0-9a-f]+) row=(-?\d+) count=(\d+)", r.stdout)
    assert len(got) == 10
    for b, fam, mx, row, count in got:
        s = summary[int(b)][["dyn_ang", "dyn_lin", "rom", "terrain", "force"].index(fam)]
        assert (int(mx, 16), int(row), int(count)) == (int(bits(s["max"]).reshape(-1)[0]), int(s["row"]), int(s["count"])), (b, fam, s)


def test_shifted_windows_accumulate_what_they_executed():
    """B = 2, two replans behind the first plan and finish(): check_worst() is the numpy accumulate of table-mode summaries over
    the executed ranges; plans and trajectory rows are the same bits with and without the check."""
    import torch
    from qtos_amd import capi, plan_check as pc, workloads
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
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, check=capi.check_params(tol=pcc.TOL))
        runs = {}
        for on in (False, True):
            W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=seg / 1000.0, search=0.0, trajectory=cap,
                               check=capi.check_params(tol=pcc.TOL) if on else None)
            W.replan()
            torch.cuda.synchronize()
            handed = []
            for _ in range(2):
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor), first=0, n=seg))
                W.replan()
                torch.cuda.synchronize()
                assert (host(W.row) == seg).all()
            mid = W.check_worst().copy() if on else None
            n_all = int(round(cfg.duration * 1000.0)) + 1
            first = 0
            while first < n_all:
                n = min(n_all - first, cap)
                handed.append(dict(nodes=host(W.nodes), t0=host(W.t0), cursor=host(W.cursor) + first, first=first, n=n))
                first += n
            W.finish()
            torch.cuda.synchronize()
            if not on:
                assert W._check is None and not hasattr(W, "check_summary")
                with pytest.raises(RuntimeError):
                    W.check_worst()
            runs[on] = dict(handed=handed, mid=mid, end=W.check_worst().copy() if on else None, traj=host(W.traj), cursor=host(W.cursor),
                            t0=host(W.t0), nodes=host(W.nodes))
        a, b = runs[False], runs[True]
        for key in ("traj", "t0", "nodes"):
            assert np.array_equal(bits(a[key]), bits(b[key])), key
        assert np.array_equal(a["cursor"], b["cursor"])
        want = pc.empty_summary(B)
        for i, h in enumerate(b["handed"]):
            p = capi.check_params(hz=1000.0, first_row=h["first"], n_rows=h["n"], tol=pcc.TOL)
            _, s = P.plan_check(h["nodes"], h["t0"], p, cursor=h["cursor"], rows=False)
            want = pc.accumulate(want, s)
            if i == 1:
                assert b["mid"].tobytes() == want.tobytes(), (b["mid"], want)
        assert b["end"].tobytes() == want.tobytes(), (b["end"], want)
        assert (b["end"]["count"][:, 1] > 0).all() and (b["end"]["row"] >= 0).all()
        pcc.record("gpu_shifted_windows", dict(dyn_lin_max=[float(v) for v in b["end"]["max"][:, 1]],
                                               dyn_ang_max=[float(v) for v in b["end"]["max"][:, 0]]))
    finally:
        P.close()


def test_solve_and_command_line_print_the_check(tmp_path):
    """LocalPlanner.solve(check=...) writes one line per family behind the solve and keeps the records; `python -m qtos_amd.main
    ... --check` prints the same lines in front of the status line; CSV and exit status are what they are without it."""
    import io
    import sys
    from conftest import load_gv
    from qtos_amd import capi, flags, plan_check as pc
    from qtos_amd.planner import LocalPlanner
    inp = load_gv("gv1")["inputs"]
    args = {"-g": inp["g"], "-s": inp["s"], "-s_ang": [0, 0, 0], "-e1": inp["ee"][0], "-e2": inp["ee"][1],
            "-e3": inp["ee"][2], "-e4": inp["ee"][3], "-t": 3.756, "-resolution": 0.01, "scripts": {}}
    lp = LocalPlanner(max_batch=1)
    try:
        buf = io.StringIO()
        assert lp.solve(args, out_csv=str(tmp_path / "a.csv"), check=buf) == 0
        lines = buf.getvalue().splitlines()
        summary = lp.last["check"]
        assert len(lines) == 5 and [ln.split()[2] for ln in lines] == list(pc.FAMILIES)
        assert lines == pc.report_lines(summary, 3.756, 1000.0, capi.CHECK_TOL)
        rows, want = lp.planner().plan_check(lp.last["nodes"][:1], 3.756, capi.check_params(n_rows=5001))
        assert summary.tobytes() == want[0].tobytes() == pc.summarise(rows[0], 0, pc.stance_rows(_layout(lp.cfg), 1000.0, 0, 5001),
                                                                      capi.CHECK_TOL).tobytes()
        assert summary["max"][1] > 1.0 and lp.last["viol"][0] <= 1e-4                    # newtons between the knots of a solved plan
        assert lp.solve(args, out_csv=str(tmp_path / "b.csv")) == 0 and "check" not in lp.last
    finally:
        lp.close()
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "qtos_amd.main"] + flags.cmd_args(args).split() + ["--out", str(tmp_path / "c.csv"), "--check"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert out[-1] == "status -> 0" and out[-6:-1] == lines
    assert open(tmp_path / "c.csv", "rb").read() == open(tmp_path / "a.csv", "rb").read()


def _layout(cfg):
    from oracle import splines as sp
    return sp.layout(cfg)
