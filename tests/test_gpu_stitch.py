"""The stitch kernel of the receding windows on the MI355X (pytest -m gpu): k_stitch's rows against qtos_sample_csv's tables (to the
bit), its ring against stitcher.ring_append, counts at the tile's edges and beyond the ring, the host form against the device form,
the argument checks, the ShiftedWindows loop with a trajectory ring against the numpy statement of the rule
(stitcher.stitch_segments) and against the loop without a ring, and the loop from plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")

B, HZ = 8, 1000.0
TILE = 512                                                       # rows per tile of k_stitch (STITCH_TILE, window_kernels.hpp)
COUNTS = [0, 1, 255, 256, 257, 2500, 5001, 5300]                 # an empty window ... beyond the plan's last row (5000)
COUNTS_TILE = [TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE, 2 * TILE + 1, 37, 5999]
SENTINEL = -98765.4321


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


class Plans:
    """Eight trot plans on flat ground (one small solve for the module) and what the tests share."""

    def __init__(self):
        import torch
        from qtos_amd import workloads
        from qtos_amd.capi import Planner
        from qtos_amd.config import PlannerConfig
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.P = Planner(PlannerConfig.knots100(gait="trot"), max_batch=B)
        start, goal = workloads.flat_goals(B, seed=7)
        self.nodes, status, _, _ = self.P.plan(start, goal)
        assert (status == 0).all(), status
        self.t0 = 3.756 * np.arange(B)
        self.n_table = 6001                                      # rows 0 .. 6000: first_row 1 + the largest count fit
        self.table = self.P.sample(self.nodes, self.t0, n_rows=self.n_table)
        self.table.setflags(write=False)
        self.d_nodes = torch.as_tensor(self.nodes, dtype=torch.float64, device=self.dev).contiguous()

    def sample(self, t0, n_rows):
        return self.P.sample(self.nodes, t0, n_rows=n_rows)

    def device(self, ring, cursor, t0, counts, first_row, n_scalar=0, advance=True, expect=0):
        """qtos_stitch_device on copies of the host arrays; returns (ring, cursor, t0) as numpy."""
        from qtos_amd import capi
        torch = self.torch
        t_ring = torch.as_tensor(np.ascontiguousarray(ring), dtype=torch.float64, device=self.dev)
        t_cur = torch.as_tensor(np.ascontiguousarray(cursor, np.int64), device=self.dev)
        t_t0 = torch.as_tensor(np.ascontiguousarray(t0, np.float64), device=self.dev)
        t_n = None if counts is None else torch.as_tensor(np.ascontiguousarray(counts, np.int32), device=self.dev)
        s = capi.stitch_params(ring.shape[1], first_row, n_scalar, HZ, advance)
        torch.cuda.synchronize()
        rc = self.P.lib.qtos_stitch_device(self.P.h, B, C.byref(s), self.d_nodes.data_ptr(), None if t_n is None else t_n.data_ptr(),
                                           t_t0.data_ptr(), t_ring.data_ptr(), t_cur.data_ptr(),
                                           C.c_void_p(torch.cuda.current_stream(self.dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == expect, (rc, self.P.lib.qtos_last_error(self.P.h))
        return t_ring.cpu().numpy(), t_cur.cpu().numpy(), t_t0.cpu().numpy()


@pytest.fixture(scope="module")
def plans():
    p = Plans()
    yield p
    p.P.close()


def segments_expected(table, counts, first_row, cap):
    """The ring after one call from cursor 0, written out with slices (not through ring_append)."""
    want = np.full((B, cap, 37), SENTINEL)
    for b, n in enumerate(counts):
        n = min(max(int(n), 0), cap)
        want[b, :n] = table[b, first_row:first_row + n]
    return want


@pytest.mark.parametrize("first_row", [0, 1])
def test_segments_are_the_sampled_rows_and_nothing_else_is_written(plans, first_row):
    cap = 6000
    empty = np.full((B, cap, 37), SENTINEL)
    last = int(round(plans.P.dims.duration * HZ))
    assert last == 5000 and first_row + max(COUNTS + COUNTS_TILE) <= plans.n_table
    for counts in (COUNTS, COUNTS_TILE):
        want = segments_expected(plans.table, counts, first_row, cap)
        ring, cursor, t0 = plans.device(empty, np.zeros(B, np.int64), plans.t0, counts, first_row, advance=True)
        diff = bits(ring) != bits(want)
        print("[k_stitch] first_row %d counts %s: %d rows written, %d cells differ" % (first_row, counts, sum(counts), int(diff.sum())))
        assert not diff.any(), np.argwhere(diff)[:5]
        assert int((ring == SENTINEL).all(axis=2).sum()) == B * cap - sum(counts)       # every other row holds the sentinel
        assert cursor.dtype == np.int64 and cursor.tolist() == counts
        assert np.array_equal(bits(t0), bits(plans.t0 + np.asarray(counts, np.float64) / HZ))
        # without the clock: the same ring and cursor, t0 as it was
        ring0, cursor0, t00 = plans.device(empty, np.zeros(B, np.int64), plans.t0, counts, first_row, advance=False)
        assert np.array_equal(bits(ring0), bits(want)) and cursor0.tolist() == counts
        assert np.array_equal(bits(t00), bits(plans.t0))
    # beyond the plan's end (plan rows 5001 ..: k / hz > T, the sampler clamps the plan time to T; T itself need not be
    # 5000 / hz to the bit) the rows repeat one state under time stamps that go on
    b = COUNTS.index(5300)
    ring, _, _ = plans.device(empty, np.zeros(B, np.int64), plans.t0, COUNTS, first_row, advance=False)
    tail = ring[b, last + 1 - first_row:5300]
    assert len(tail) >= 298
    assert np.array_equal(bits(tail[:, 1:]), bits(np.broadcast_to(tail[0, 1:], tail[:, 1:].shape))) and (np.diff(tail[:, 0]) > 0).all()


def test_ring_wraps_like_ring_append(plans):
    from qtos_amd.stitcher import ring_append
    cap = 300
    cursor = np.array([0, 299, 300, 12345, 1, 150, 599, 2 ** 40 + 7], np.int64)
    ring = np.full((B, cap, 37), SENTINEL)
    t0 = plans.t0.copy()
    for first_row, n in ((0, 200), (1, 257), (0, 300)):
        table = plans.sample(t0, first_row + n)                  # the clock has moved: the time stamps are those of the new t0
        want, want_cur = ring.copy(), cursor.copy()
        for b in range(B):
            want_cur[b] = ring_append(want[b], cursor[b], table[b, first_row:first_row + n])
        ring, cursor, t0_new = plans.device(ring, cursor, t0, [n] * B, first_row, advance=True)
        assert np.array_equal(bits(ring), bits(want)), (first_row, n)
        assert np.array_equal(cursor, want_cur)
        assert np.array_equal(bits(t0_new), bits(t0 + n / HZ))
        t0 = t0_new
    assert not (ring == SENTINEL).any()                          # (the last call filled every ring)


def test_scalar_count_clamp_and_negative_counts(plans):
    from qtos_amd.stitcher import ring_append
    cap = 300
    empty = np.full((B, cap, 37), SENTINEL)
    zero = np.zeros(B, np.int64)
    # d_n_rows NULL: n_rows for every window
    ring, cursor, t0 = plans.device(empty, zero, plans.t0, None, 1, n_scalar=100)
    assert np.array_equal(bits(ring), bits(segments_expected(plans.table, [100] * B, 1, cap))) and cursor.tolist() == [100] * B
    assert np.array_equal(bits(t0), bits(plans.t0 + 100 / HZ))
    # counts above the capacity write exactly `capacity` rows, negative ones nothing
    counts = [301, 1000, 300, 299, -1, -5, 0, 2 ** 31 - 1]
    cur0 = np.array([0, 7, 299, 300, 5, 6, 7, 1234], np.int64)
    n_eff = [300, 300, 300, 299, 0, 0, 0, 300]
    want = empty.copy()
    for b in range(B):
        assert ring_append(want[b], cur0[b], plans.table[b, 0:n_eff[b]]) == cur0[b] + n_eff[b]
    ring, cursor, t0 = plans.device(empty, cur0, plans.t0, counts, 0)
    assert np.array_equal(bits(ring), bits(want))
    assert np.array_equal(cursor, cur0 + np.asarray(n_eff))
    assert np.array_equal(bits(t0), bits(plans.t0 + np.asarray(n_eff, np.float64) / HZ))
    assert (ring[4:7] == SENTINEL).all() and int((ring[3] == SENTINEL).all(axis=1).sum()) == 1
    # the scalar form clamps too
    ring, cursor, _ = plans.device(empty, cur0, plans.t0, None, 0, n_scalar=5000)
    want = empty.copy()
    for b in range(B):
        ring_append(want[b], cur0[b], plans.table[b, 0:cap])
    assert np.array_equal(bits(ring), bits(want)) and np.array_equal(cursor, cur0 + cap)


@pytest.mark.parametrize("first_row", [0, 1])
def test_host_form_leaves_what_the_device_form_leaves(plans, first_row):
    cap = 6000
    empty = np.full((B, cap, 37), SENTINEL)
    zero = np.zeros(B, np.int64)
    dev = plans.device(empty, zero, plans.t0, COUNTS, first_row)
    ring, cursor, t0 = plans.P.stitch(plans.nodes, COUNTS, plans.t0, empty, zero, first_row=first_row, hz=HZ, advance_clock=True)
    assert (empty == SENTINEL).all() and (zero == 0).all()       # (Planner.stitch returns new arrays)
    assert np.array_equal(bits(ring), bits(dev[0])) and np.array_equal(cursor, dev[1]) and np.array_equal(bits(t0), bits(dev[2]))
    assert np.array_equal(bits(ring), bits(segments_expected(plans.table, COUNTS, first_row, cap)))
    # the scalar count and the clock left alone
    dev = plans.device(empty, zero + 11, plans.t0, None, first_row, n_scalar=123, advance=False)
    host = plans.P.stitch(plans.nodes, 123, plans.t0, empty, zero + 11, first_row=first_row, advance_clock=False)
    assert np.array_equal(bits(host[0]), bits(dev[0])) and np.array_equal(host[1], dev[1]) and host[1].tolist() == [134] * B
    assert np.array_equal(bits(host[2]), bits(plans.t0))


def test_bad_arguments_answer_minus_one_and_run_no_kernel(plans):
    from qtos_amd import capi
    torch, P, dev = plans.torch, plans.P, plans.dev
    cap = 64
    t_ring = torch.full((B, cap, 37), SENTINEL, dtype=torch.float64, device=dev)
    t_cur = torch.full((B,), 5, dtype=torch.int64, device=dev)
    t_t0 = torch.as_tensor(plans.t0, dtype=torch.float64, device=dev)
    t_n = torch.full((B,), 3, dtype=torch.int32, device=dev)
    h_ring, h_cur, h_t0, h_n = np.full((B, cap, 37), SENTINEL), np.full(B, 5, np.int64), plans.t0.copy(), np.full(B, 3, np.int32)
    llp = C.POINTER(C.c_longlong)
    good = capi.stitch_params(cap, 0, 3)

    def device(p=P.h, b=B, s=good, nodes=plans.d_nodes.data_ptr(), n=t_n.data_ptr(), t0=t_t0.data_ptr(), ring=t_ring.data_ptr(),
               cur=t_cur.data_ptr()):
        return P.lib.qtos_stitch_device(p, b, None if s is None else C.byref(s), nodes, n, t0, ring, cur, None)

    def host(p=P.h, b=B, s=good, nodes=capi._dp(plans.nodes), n=capi._ip(h_n), t0=capi._dp(h_t0), ring=capi._dp(h_ring),
             cur=h_cur.ctypes.data_as(llp)):
        return P.lib.qtos_stitch(p, b, None if s is None else C.byref(s), nodes, n, t0, ring, cur)

    def params(**kw):
        s = capi.stitch_params(cap, 0, 3)
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    torch.cuda.synchronize()
    for name, call in (("device", device), ("host", host)):
        got = {
            "null planner": call(p=None), "B = 0": call(b=0), "B < 0": call(b=-3), "null params": call(s=None),
            "null nodes": call(nodes=None), "null t0": call(t0=None), "null traj": call(ring=None), "null cursor": call(cur=None),
            "capacity 0": call(s=params(capacity=0)), "capacity < 0": call(s=params(capacity=-1)),
            "first_row -1": call(s=params(first_row=-1)), "first_row 1000001": call(s=params(first_row=1000001)),
            "n_rows < 0 without d_n_rows": call(s=params(n_rows=-1), n=None),
        }
        assert all(v == -1 for v in got.values()), (name, got)
        # on the edge of the checks: accepted
        assert call(s=params(first_row=1000000, n_rows=-1)) == 0, name      # (n_rows is not read where d_n_rows is given)
    torch.cuda.synchronize()
    # nothing ran for the bad calls: the one good call of each form moved its cursor by 3, everything else is as it was
    assert t_cur.cpu().tolist() == [8] * B and h_cur.tolist() == [8] * B
    ring = t_ring.cpu().numpy()
    assert int((ring != SENTINEL).any(axis=2).sum()) == 3 * B and (ring[:, :5] == SENTINEL).all() and (ring[:, 8:] == SENTINEL).all()
    assert np.array_equal(bits(ring), bits(h_ring))


def _window_starts(maps, cell):
    from qtos_amd import workloads
    start, goal, map_id = workloads.mpc_goals(B, seed=5, terrains=(maps, cell))
    return start, goal - start[:, 0:3], map_id


def _loop(handover, trajectory, stitch, replans=3):
    """The cold plan, `replans` replans and finish(); what every replan handed over from, and the results."""
    import torch
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    maps, cell = workloads.random_terrains()
    start, step, map_id = _window_starts(maps, cell)
    P = Planner(PlannerConfig.receding_windows(), max_batch=B)
    try:
        P.set_heightfields(maps, cell)
        W = ShiftedWindows(P, start, step, map_id, advance=2.5, x_range=(0.0, 2.2), handover=handover, trajectory=trajectory,
                           stitch=stitch)
        assert (W.traj is None) == (trajectory is None)
        host = lambda t: t.cpu().numpy().copy()
        W.replan()
        torch.cuda.synchronize()
        out = dict(plans=[dict(nodes=host(W.nodes), status=host(W.status), iters=host(W.iters))], handed=[])
        for _ in range(replans):
            before = dict(nodes=host(W.nodes), t0=host(W.t0))
            W.replan()
            torch.cuda.synchronize()
            if trajectory is not None:
                before["row"] = host(W.row)
            out["handed"].append(before)
            out["plans"].append(dict(nodes=host(W.nodes), status=host(W.status), iters=host(W.iters)))
        if trajectory is not None:
            W.finish()
            n_all = int(round(P.dims.duration * W.hz)) + 1
            out["t0"], out["cursor"] = host(W.t0), host(W.cursor)
            out["tables"] = [P.sample(h["nodes"], h["t0"], n_rows=n_all) for h in out["handed"]]
            out["last_table"] = P.sample(out["plans"][-1]["nodes"], out["t0"], n_rows=n_all)
            out["rows"] = [W.trajectory_rows(b) for b in range(B)]
        else:
            with pytest.raises(RuntimeError):
                W.finish()
            assert (host(W.t0) == 0).all()
        return out
    finally:
        P.close()


_plain = {}


@pytest.mark.parametrize("handover", ["kernel", "rows"])
@pytest.mark.parametrize("stitch,first_row", [("clean", 0), ("reference", 1)])
def test_loop_keeps_the_executed_trajectory_and_disturbs_nothing(handover, stitch, first_row):
    from qtos_amd.stitcher import stitch_segments
    cap = 9000
    got = _loop(handover, cap, stitch)
    if handover not in _plain:
        _plain[handover] = _loop(handover, None, "clean")
    # stitching disturbs nothing: the plans of the loop without a ring, to the bit
    for k, (a, b) in enumerate(zip(got["plans"], _plain[handover]["plans"])):
        assert np.array_equal(bits(a["nodes"]), bits(b["nodes"])), k
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"]), k
    # the windows' clock: t0 of a plan is t0 of the plan before + its hand-over row / hz
    t0 = np.zeros(B)
    for h in got["handed"]:
        assert np.array_equal(bits(h["t0"]), bits(t0))
        assert ((h["row"] >= 2500) & (h["row"] <= 2900)).all()
        t0 = t0 + h["row"] / 1000.0
    assert np.array_equal(bits(got["t0"]), bits(t0))
    n_all = got["last_table"].shape[1]
    total = sum(h["row"].astype(np.int64) for h in got["handed"]) + n_all - first_row
    assert np.array_equal(got["cursor"], total) and (total > cap).all()          # (the rings have wrapped)
    for b in range(B):
        want = np.concatenate([stitch_segments([t[b] for t in got["tables"]], [h["row"][b] for h in got["handed"]], first_row),
                               got["last_table"][b, first_row:]], axis=0)
        assert len(want) == total[b]
        rows = got["rows"][b]
        assert rows.shape == (cap, 37)
        assert np.array_equal(bits(rows), bits(want[-cap:])), (b, int((bits(rows) != bits(want[-cap:])).sum()))
        if stitch == "clean":
            assert np.abs(np.diff(rows[:, 0]) - 1e-3).max() < 1e-9, b
    print("[loop %s %s] hand-over rows %s, cursors %s" % (handover, stitch, [h["row"].tolist() for h in got["handed"]], got["cursor"].tolist()))


def test_c_loop_stitches_three_replans(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "stitch_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "stitch_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), str(img)], capture_output=True, text=True, timeout=330)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_stitch=%d stitch_null=-1 stitch_device_null=-1" % C.sizeof(capi.QtosStitch)
    assert lines[1] == "bad_args=-1,-1,-1,-1,-1,-1"
    assert lines[2].startswith("cold rc=0 status=0,0 ")
    recs = [dict(t.split("=") for t in ln.split()) for ln in lines[3:9]]
    assert [(int(q["replan"]), int(q["window"])) for q in recs] == [(r_, b) for r_ in (1, 2, 3) for b in (0, 1)]
    cursor, t0 = {0: 0, 1: 0}, {0: 0.0, 1: 10.0}
    for q in recs:
        b = int(q["window"])
        assert int(q["handover"]) == 0 and int(q["stitch"]) == 0 and int(q["plan"]) == 0 and int(q["status"]) == 0, q
        assert 2500 <= int(q["row"]) <= 2900, q
        cursor[b] += int(q["row"])
        t0[b] = t0[b] + int(q["row"]) / 1000.0
        assert int(q["cursor"]) == cursor[b] and float(q["t0"]) == t0[b], q
    assert lines[9] == "finish rc=0 rows=5001"
    for b, ln in enumerate(lines[10:12]):
        q = dict(t.split("=") for t in ln.split())
        assert int(q["window"]) == b and int(q["cursor"]) == cursor[b] + 5001 and int(q["increasing"]) == 1, q
        assert float(q["first_t"]) == 10.0 * b and float(q["last_t"]) == t0[b] + 5000 / 1000.0, q
