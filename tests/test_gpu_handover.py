"""The hand-over kernel of the receding windows on the MI355X (pytest -m gpu): k_handover against the numpy statement of its rule
on sampled row tables (to the bit), the ShiftedWindows loop with the kernel against the loop through the row table (to the bit),
host form against device form, the reference's height-set rule against the host Stitcher, and the loop from plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def contact_mask(rows, rule, heights):
    """[B, n_rows]: the rule on every row of a table, written out once more (not through handover_index)."""
    if rule == 0:
        return (rows[:, :, [27, 30, 33, 36]] > 0).all(axis=2)
    z6 = np.rint(rows[:, :, [9, 12, 15, 18]] * 1e6)
    return np.isin(z6, np.rint(np.asarray(heights, np.float64) * 1e6)).all(axis=2)


def _terrain_plans(B):
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    maps, cell = workloads.random_terrains()
    P = Planner(PlannerConfig.receding_windows(), max_batch=B)
    P.set_heightfields(maps, cell)
    start, goal, map_id = workloads.mpc_goals(B, seed=5, terrains=(maps, cell))
    nodes, status, _, _ = P.plan(start, goal, map_id)
    # eight terrain levels: those the windows' feet start on first, then the maps' lowest others
    own = np.unique(start[:, [8, 11, 14, 17]])
    levels = list(own[:8]) + [v for v in np.unique(maps) if v not in own]
    heights = tuple(float(v) for v in levels[:8])
    return P, nodes, status, heights


def _trot_plans(B):
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    P = Planner(PlannerConfig.knots100(gait="trot"), max_batch=B)
    start, goal = workloads.flat_goals(B, seed=7)
    nodes, status, _, _ = P.plan(start, goal)
    return P, nodes, status, (0.0,)


@pytest.mark.parametrize("workload", ["random_terrains", "flat_trot"])
def test_kernel_picks_and_evaluates_the_rows_of_the_numpy_statement(workload):
    from qtos_amd.replan import handover_index
    B, hz = 64, 1000.0
    P, nodes, status, heights = (_terrain_plans if workload == "random_terrains" else _trot_plans)(B)
    try:
        assert (status == 0).sum() >= B - 2, status
        table = P.sample(nodes, 0.0)                         # the whole plans: every row the kernel can pick
        n_all = table.shape[1]
        assert n_all == int(round(P.dims.duration * hz)) + 1
        # a search so short that a window has no passing candidate: 20 rows from the first row behind 2 s at which window 0
        # starts a stretch of 21 rows without contact (read from the table, per rule)
        cases = []
        for rule in (0, 1):
            ok0 = contact_mask(table[:1], rule, heights)[0]
            free = [k for k in range(2000, n_all - 21) if not ok0[k:k + 21].any()]
            assert free, "no stretch of 21 rows without contact in window 0"
            cases += [(rule, 2500, 400, False), (rule, free[0], 20, True)]
        for rule, k0, n_search, expect_empty in cases:
            ok = contact_mask(table, rule, heights)[:, k0:k0 + n_search + 1]
            n_empty = int((~ok.any(axis=1)).sum())
            if expect_empty:
                assert n_empty >= 1
            want = handover_index(table, k0, n_search, rule, heights)
            assert np.array_equal(want, np.where(ok.any(axis=1), k0 + ok.argmax(axis=1), k0))
            for zf in (False, True):
                start, offset, row = P.handover(nodes, advance=k0 / hz, search=n_search / hz, hz=hz, rule=rule, heights=heights,
                                                zero_filter=zf)
                print("[k_handover %s] rule %d k0 %d search %d zero_filter %d: rows %d .. %d, %d windows without a candidate, "
                      "%d distinct rows" % (workload, rule, k0, n_search, zf, row.min(), row.max(), n_empty, len(set(row.tolist()))))
                assert np.array_equal(row.astype(np.int64), want), (rule, k0, np.nonzero(row != want)[0][:8])
                ref = table[np.arange(B), want, 1:25].copy()
                if zf:
                    assert ((np.abs(ref) < 1e-4) & (ref != 0)).any()      # (the filter has something to do)
                    ref[np.abs(ref) < 1e-4] = 0.0
                assert np.array_equal(bits(start), bits(ref))
                assert np.array_equal(bits(offset), bits(want.astype(np.float64) / hz))
    finally:
        P.close()


def _window_starts(B, maps, cell, n_far):
    """mpc_goals' windows; the last n_far of them stand near the far end of their 2.2 m map instead (they turn round at once)."""
    from qtos_amd import heightfield, workloads
    start, goal, map_id = workloads.mpc_goals(B, seed=5, terrains=(maps, cell))
    step = goal - start[:, 0:3]
    for b, x in zip(range(B - n_far, B), np.linspace(1.9, 2.15, n_far)):
        feet = workloads.NOMINAL_FEET + np.array([x, 0.0, 0.0])
        fz = heightfield.height_at(maps[map_id[b]], cell, feet[:, 0], feet[:, 1], mode=1)
        start[b] = workloads.rest_start(x, 0.0, 0.24 + float(heightfield.height_at(maps[map_id[b]], cell, x, 0.0, mode=1)), fz)
    return start, step, map_id


def test_loop_with_the_kernel_gives_the_bits_of_the_loop_through_the_row_table():
    import torch
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    B, K = 64, 5
    cfg = PlannerConfig.receding_windows()
    maps, cell = workloads.random_terrains()
    start, step, map_id = _window_starts(B, maps, cell, n_far=16)
    runs = {}
    for mode in ("rows", "kernel"):
        P = Planner(cfg, max_batch=B)
        try:
            P.set_heightfields(maps, cell)
            W = ShiftedWindows(P, start, step, map_id, advance=2.5, x_range=(0.0, 2.2), handover=mode)
            assert W.handover == mode and hasattr(W, "rows") == (mode == "rows")
            snaps = []
            for k in range(K + 1):                            # the cold plan, then K replans
                W.replan()
                torch.cuda.synchronize()
                snaps.append({n: getattr(W, n).cpu().numpy().copy() for n in ("start", "goal", "goal_step", "offset", "nodes", "status", "iters")})
            runs[mode] = snaps
        finally:
            P.close()
    turns = sum(int((np.sign(a["goal_step"][:, 0]) != np.sign(b["goal_step"][:, 0])).sum())
                for a, b in zip(runs["rows"][:-1], runs["rows"][1:]))
    print("[loop] %d windows x %d replans: %d turn-arounds, offsets %.3f .. %.3f s, converged %d of %d" %
          (B, K, turns, min(s["offset"].min() for s in runs["rows"][1:]), max(s["offset"].max() for s in runs["rows"][1:]),
           sum(int((s["status"] == 0).sum()) for s in runs["rows"]), B * (K + 1)))
    assert turns >= 1
    for k, (a, b) in enumerate(zip(runs["rows"], runs["kernel"])):
        for n in ("start", "goal", "goal_step", "offset", "nodes"):
            assert np.array_equal(bits(a[n]), bits(b[n])), (k, n, int((bits(a[n]) != bits(b[n])).sum()))
        assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["iters"], b["iters"]), k


def test_host_form_device_form_and_no_trace_on_the_handle():
    import torch
    from qtos_amd import capi, workloads
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.knots100(gait="trot")
    B = 16
    start, goal = workloads.flat_goals(B, seed=4)
    P, Q = capi.Planner(cfg, max_batch=B), capi.Planner(cfg, max_batch=B)
    try:
        first = P.plan(start, goal)
        nodes = first[0]
        gs = np.tile([0.4, 0.01, 0.0], (B, 1))
        gs[::3, 0] *= -1.0
        gl = np.tile([9.0, 9.0, 0.24], (B, 1))
        x_range = (0.3, 1.5)                                  # (starts are spread over 0 .. 2 m: windows beyond either end)
        host = P.handover(nodes, advance=2.5, search=0.4, rule="heights", heights=(0.0,), zero_filter=True, goal_step=gs, goal=gl,
                          x_range=x_range)
        dev = torch.device("cuda", 0)
        f64 = dict(dtype=torch.float64, device=dev)
        t_nodes, t_gs, t_gl = (torch.as_tensor(np.ascontiguousarray(a), **f64) for a in (nodes, gs, gl))
        t_start, t_off = torch.empty((B, 24), **f64), torch.empty((B,), **f64)
        t_row = torch.empty((B,), dtype=torch.int32, device=dev)
        h = capi.handover_params(2.5, 0.4, 1000.0, "heights", (0.0,), True, x_range)
        torch.cuda.synchronize()
        rc = P.lib.qtos_handover_device(P.h, B, C.byref(h), t_nodes.data_ptr(), t_gs.data_ptr(), t_start.data_ptr(), t_gl.data_ptr(),
                                        t_off.data_ptr(), t_row.data_ptr(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        for a, b in zip(host, (t_start, t_off, t_row, t_gs, t_gl)):
            b = b.cpu().numpy()
            assert np.array_equal(a.view(np.int64) if a.dtype == np.float64 else a, b.view(np.int64) if b.dtype == np.float64 else b)
        st, off, row, gs2, gl2 = host
        assert (row >= 2500).all() and (row <= 2900).all() and np.array_equal(off, row / 1000.0)
        sgn = np.where(st[:, 0] > x_range[1], -1.0, np.where(st[:, 0] < x_range[0], 1.0, np.sign(gs[:, 0])))
        assert (sgn != np.sign(gs[:, 0])).any()               # some window really turns round
        assert np.array_equal(gs2[:, 0], sgn * np.abs(gs[:, 0])) and np.array_equal(gs2[:, 1:], gs[:, 1:])
        assert np.array_equal(gl2[:, 0:2], st[:, 0:2] + gs2[:, 0:2]) and (gl2[:, 2] == 0.24).all()
        assert not ((np.abs(st) < 1e-4) & (st != 0)).any()
        # bad arguments with a planner
        bad = capi.handover_params(6.0, 0.4)
        assert P.lib.qtos_handover_device(P.h, B, C.byref(bad), t_nodes.data_ptr(), None, t_start.data_ptr(), None, t_off.data_ptr(), None, None) == -1
        assert P.lib.qtos_handover_device(P.h, B, C.byref(h), t_nodes.data_ptr(), t_gs.data_ptr(), t_start.data_ptr(), None, t_off.data_ptr(), None, None) == -1
        # the hand-over leaves no trace: the next plan call returns the bits of the call without it
        second = P.plan(start, goal)
        never = Q.plan(start, goal)
        Q.plan(start, goal)
        for x, y, z in zip(first, second, never):
            assert np.array_equal(x, y) and np.array_equal(x, z)
        assert P.totals() == Q.totals() and P.totals()[1] == 2 * int(first[2].sum())
        assert P.timing_detail()["pattern_calls"] == Q.timing_detail()["pattern_calls"]
        # between submit and the end of wait the host form answers -5
        tin = [torch.as_tensor(np.ascontiguousarray(x), device=dev) for x in (start, goal)]
        out = (torch.empty((B, P.n), **f64), torch.empty(B, dtype=torch.int32, device=dev),
               torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, **f64))
        s2 = torch.cuda.Stream(dev)
        torch.cuda.synchronize()
        o_st, o_off = np.empty((B, 24)), np.empty(B)
        P.submit(B, tin[0].data_ptr(), tin[1].data_ptr(), None, None, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                 out[3].data_ptr(), s2.cuda_stream)
        rc = P.lib.qtos_handover(P.h, B, C.byref(h), capi._dp(nodes), None, capi._dp(o_st), None, capi._dp(o_off), None)
        P.wait()
        s2.synchronize()
        assert rc == -5
        assert np.array_equal(out[0].cpu().numpy(), first[0])
        again = P.handover(nodes, advance=2.5, search=0.4, rule="heights", heights=(0.0,), zero_filter=True)
        assert np.array_equal(again[0].view(np.int64), st.view(np.int64)) and np.array_equal(again[2], row)
    finally:
        P.close()
        Q.close()


@pytest.mark.parametrize("advance", [2.5, 3.75])
def test_height_set_rule_hands_over_where_the_stitcher_does(advance):
    import torch
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    from qtos_amd.replan import ShiftedWindows
    from qtos_amd.stitcher import Stitcher
    B = 8
    P = Planner(PlannerConfig.reference_compat(), max_batch=B)
    try:
        start, goal = workloads.flat_goals(B, seed=11)
        with pytest.raises(ValueError):
            ShiftedWindows(P, start, goal - start[:, 0:3], advance=advance, handover="rows", contact="heights")
        W = ShiftedWindows(P, start, goal - start[:, 0:3], advance=advance, handover="kernel", contact="heights", height_set=(0.0,))
        W.replan()
        torch.cuda.synchronize()
        assert bool((W.status == 0).all())
        table = P.sample(W.nodes.cpu().numpy(), 0.0)
        W.replan()
        torch.cuda.synchronize()
        row = W.row.cpu().numpy()
        k0 = int(round(advance * 1000))
        want = []
        for b in range(B):
            st = Stitcher(lookahead=k0, height_set=(0.0,))
            st.state(np.round(table[b], 6), 0.0)
            want.append(st.lookahead)
        print("[heights] advance %.2f: kernel rows %s, Stitcher %s" % (advance, row.tolist(), want))
        assert row.tolist() == want and all(k0 <= r <= k0 + 400 for r in want)
        assert np.array_equal(bits(W.start.cpu().numpy()), bits(table[np.arange(B), row, 1:25]))
        assert np.array_equal(bits(W.offset.cpu().numpy()), bits(row / 1000.0))
    finally:
        P.close()


def test_c_loop_replans_three_times(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "replan_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "replan_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), str(img)], capture_output=True, text=True, timeout=330)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_handover=%d handover_null=-1 handover_device_null=-1" % C.sizeof(capi.QtosHandover)
    assert lines[1] == "bad_args=-1,-1,-1,-1,-1,-1"
    assert lines[2].startswith("cold rc=0 status=0,0 ")
    recs = [dict(t.split("=") for t in ln.split()) for ln in lines[3:]]
    assert [(int(q["replan"]), int(q["window"])) for q in recs] == [(r_, b) for r_ in (1, 2, 3) for b in (0, 1)]
    x = {0: 0.0, 1: 0.1}
    for q in recs:
        assert int(q["handover"]) == 0 and int(q["plan"]) == 0 and int(q["status"]) == 0, q
        assert 2500 <= int(q["row"]) <= 2900 and float(q["offset"]) == int(q["row"]) / 1000.0, q
        s = [float(v) for v in q["start"].split(",")]
        assert s[0] > x[int(q["window"])] + 0.05 and abs(s[1]) < 0.05 and 0.15 < s[2] < 0.35, q     # the robots walk on
        x[int(q["window"])] = s[0]
