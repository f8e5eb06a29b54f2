"""The probe and stamp kernels of the windows' boolean maps on the MI355X (pytest -m gpu): k_probe and k_probe_stamp against the
numpy statement of their rule (feasibility.probe_table / stamp_table, which tests/test_probe_cpu.py holds to the host route) to
the bit, on the batches that file builds -- with room for every problem and with less --, the golden map's 48 fixture patches, the
host forms, the argument checks, the whole route feasibility_maps_device against feasibility_map on the golden map, its tensor
in qtos_path_plan_device and ShiftedWindows.repath, and the caller in plain C."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_probe_cpu import FIX, bits, golden_map, gpu_batch, same, stamp_cases

pytestmark = pytest.mark.gpu
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
PATTERN, IPATTERN = -98765.4321, -77
PAD = 3                                       # rows behind the last problem: the pattern stays there
OUT_F, OUT_I = ("start", "goal"), ("offsets", "slot", "patch", "map_id")


@pytest.fixture(scope="module")
def gpu():
    """One LocalPlanner / capi.Planner pair at the default configuration: the handle the host route solves on."""
    import torch
    from qtos_amd.planner import LocalPlanner
    lp = LocalPlanner(max_batch=64)
    yield torch, torch.device("cuda", 0), lp.planner(), lp
    lp.close()


def params(maps, shift, scale, **kw):
    from qtos_amd import capi
    g = capi.probe_params(np.asarray(maps), shift, scale)
    for k, v in kw.items():
        setattr(g, k, v)
    return g


def probe_device(gpu, heights, g, rows_of_room, capacity, **swap):
    """qtos_probe_device with pattern-filled outputs of `rows_of_room` problems; returns (rc, outputs as numpy).  swap: pointers
    that take the place of an array's (None: a null pointer)."""
    torch, dev, P = gpu[:3]
    maps = np.asarray(heights, float)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    n_maps, rows, cols = maps.shape
    T = dict(maps=torch.as_tensor(maps, **f64), offsets=torch.full((n_maps + 1,), IPATTERN, **i32),
             slot=torch.full((n_maps, rows, cols // 2 - 1), IPATTERN, **i32), patch=torch.full((rows_of_room, 3), IPATTERN, **i32),
             start=torch.full((rows_of_room, 24), PATTERN, **f64), goal=torch.full((rows_of_room, 3), PATTERN, **f64),
             map_id=torch.full((rows_of_room,), IPATTERN, **i32))
    ptr = {k: v.data_ptr() for k, v in T.items()}
    ptr.update(swap)
    torch.cuda.synchronize()
    rc = P.lib.qtos_probe_device(P.h, C.byref(g) if g is not None else None, ptr["maps"], capacity, ptr["offsets"], ptr["slot"], ptr["patch"],
                                 ptr["start"], ptr["goal"], ptr["map_id"], C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in T.items()}


def assert_first_rows(got, want, n):
    """offsets and slot whole, the first n problems right, the pattern intact behind them."""
    assert np.array_equal(got["offsets"], want["offsets"]) and np.array_equal(got["slot"], want["slot"])
    for k in ("patch", "map_id"):
        assert np.array_equal(got[k][:n], want[k][:n]), (k, np.argwhere(got[k][:n] != want[k][:n])[:5].tolist())
        assert (got[k][n:] == IPATTERN).all(), k
    for k in OUT_F:
        assert same(got[k][:n], want[k][:n]), (k, np.argwhere(bits(got[k][:n]) != bits(want[k][:n]))[:5].tolist())
        assert (got[k][n:] == PATTERN).all(), k


@pytest.mark.parametrize("scale", [1, 2])
def test_kernel_is_the_numpy_rule_to_the_bit(gpu, scale):
    from qtos_amd import feasibility
    maps = gpu_batch(scale)
    want = feasibility.probe_table(maps, 2, scale)
    N = len(want["patch"])
    rc, got = probe_device(gpu, maps, params(maps, 2, scale), N + PAD, N + PAD)
    assert rc == 0, gpu[2].lib.qtos_last_error(gpu[2].h)
    print("scale %d: offsets %s" % (scale, got["offsets"].tolist()))
    assert_first_rows(got, want, N)
    assert same(got["maps"], maps)
    # less room than problems: offsets and slot are whole, the first `capacity` problems right, nothing behind them
    for cap in (0, 1, N // 2, N - 1):
        rc, part = probe_device(gpu, maps, params(maps, 2, scale), N + PAD, cap)
        assert rc == 0
        assert_first_rows(part, want, cap)
    # without the optional arrays
    rc, bare = probe_device(gpu, maps, params(maps, 2, scale), N + PAD, N, start=None, goal=None, map_id=None)
    assert rc == 0 and np.array_equal(bare["patch"][:N], want["patch"]) and np.array_equal(bare["slot"], want["slot"])
    assert (bare["start"] == PATTERN).all() and (bare["goal"] == PATTERN).all() and (bare["map_id"] == IPATTERN).all()


def test_golden_map_gives_the_fixture_patches(gpu):
    from qtos_amd import feasibility
    m = golden_map()[None]
    rc, got = probe_device(gpu, m, params(m, FIX["multi_map_shift"], 1), 48 + PAD, 48 + PAD)
    assert rc == 0 and got["offsets"].tolist() == [0, 48]
    assert_first_rows(got, feasibility.probe_table(m, FIX["multi_map_shift"], 1), 48)
    for i, r in enumerate(FIX["patches"]):
        assert got["patch"][i].tolist() == [0] + r[2]
        assert same(got["start"][i, 0:2], np.array(r[0][0:2])) and same(got["goal"][i, 0:2], np.array(r[1][0:2]))
        assert same(got["start"][i, 2], np.float64(r[0][2]) + 0.24) and same(got["goal"][i, 2], np.float64(r[1][2]) + 0.24)


def stamp_device(gpu, shape, g, T, statuses, **swap):
    """qtos_probe_stamp_device on the arrays of a probe table, the map pattern-filled; returns (rc, the map's tensor)."""
    torch, dev, P = gpu[:3]
    i32 = dict(dtype=torch.int32, device=dev)
    D = dict(offsets=torch.as_tensor(T["offsets"], **i32), slot=torch.as_tensor(T["slot"], **i32),
             patch=torch.as_tensor(np.concatenate([T["patch"], np.zeros((1, 3), np.int32)]), **i32),
             status=torch.as_tensor(np.concatenate([statuses, [0]]).astype(np.int32), **i32),
             bool_maps=torch.full(tuple(shape), PATTERN, dtype=torch.float64, device=dev))
    ptr = {k: v.data_ptr() for k, v in D.items()}
    ptr.update(swap)
    torch.cuda.synchronize()
    rc = P.lib.qtos_probe_stamp_device(P.h, C.byref(g), ptr["offsets"], ptr["slot"], ptr["patch"], ptr["status"], ptr["bool_maps"],
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize()
    return rc, D["bool_maps"]


@pytest.mark.parametrize("scale", [1, 2])
def test_stamp_kernel_is_the_numpy_rule_to_the_bit(gpu, scale):
    from qtos_amd import feasibility
    for maps, shift, T, status in stamp_cases(scale):
        want = feasibility.stamp_table(maps.shape, T["offsets"], T["slot"], T["patch"], status, scale)
        rc, got = stamp_device(gpu, maps.shape, params(maps, shift, scale), T, status)
        assert rc == 0, gpu[2].lib.qtos_last_error(gpu[2].h)
        got = got.cpu().numpy()
        assert same(got, want), np.argwhere(got != want)[:5].tolist()
        assert 0 < want.sum() < want.size
        rc, bare = stamp_device(gpu, maps.shape, params(maps, shift, scale), T, status, patch=None)     # (patch is not read)
        assert rc == 0 and same(bare.cpu().numpy(), want)


def test_host_forms_leave_what_the_device_forms_leave(gpu):
    from qtos_amd import feasibility
    P = gpu[2]
    for scale in (1, 2):
        maps, shift, T, status = stamp_cases(scale)[1]
        g = params(maps, shift, scale)
        out = P.probe(maps, g)
        for k in OUT_I:
            assert np.array_equal(out[k], T[k]), k
        for k in OUT_F:
            assert same(out[k], T[k]), k
        part = P.probe(maps, g, capacity=5)
        assert np.array_equal(part["offsets"], T["offsets"]) and len(part["patch"]) == 5 and same(part["start"], T["start"][:5])
        bm = P.probe_stamp(maps.shape, out["offsets"], out["slot"], out["patch"], status, g)
        assert same(bm, feasibility.stamp_table(maps.shape, T["offsets"], T["slot"], T["patch"], status, scale))
        assert same(P.probe_stamp(maps.shape, out["offsets"], out["slot"], None, status, g), bm)
    flat = P.probe(np.zeros((5, 8)))
    assert flat["offsets"].tolist() == [0, 0] and len(flat["patch"]) == 0 and (flat["slot"] == -1).all()
    assert not P.probe_stamp((5, 8), flat["offsets"], flat["slot"], flat["patch"], np.zeros(0, np.int32)).any()
    narrow = P.probe(np.ones((4, 3)))                                           # (no candidate: the slot array is empty)
    assert narrow["offsets"].tolist() == [0, 0] and narrow["slot"].shape == (1, 4, 0)
    none = np.zeros(0, np.int32)                                                # (the stamp of it: slot and status both empty)
    assert same(P.probe_stamp((4, 3), narrow["offsets"], narrow["slot"], narrow["patch"], none),
                feasibility.stamp_table((4, 3), narrow["offsets"], narrow["slot"], narrow["patch"], none, 1))


def test_bad_arguments_answer_minus_two_and_launch_nothing(gpu):
    P = gpu[2]
    maps, shift, T, status = stamp_cases(1)[1]
    N = len(T["patch"])
    ok = lambda **kw: params(maps, shift, kw.pop("scale", 1), **kw)
    calls = [(ok(cols=1), {}), (ok(rows=0), {}), (ok(rows=129, cols=128), {}), (ok(n_maps=0), {}), (ok(scale=0), {}), (ok(scale=5), {}),
             (ok(multi_map_shift=0), {}), (ok(cell=0.0), {}), (ok(cell=float("nan")), {}), (ok(origin_shift=float("nan")), {}),
             (ok(n_maps=1 << 20, rows=16, cols=1024), {}), (ok(n_maps=(1 << 24) + 1, cols=2), {}), (None, {}), (ok(), dict(capacity=-1)), (ok(), dict(maps=None)),
             (ok(), dict(offsets=None)), (ok(), dict(slot=None)), (ok(), dict(patch=None))]
    for g, kw in calls:
        cap = kw.pop("capacity", N)
        rc, got = probe_device(gpu, maps, g, N, cap, **kw)
        assert rc == -2, (rc, kw)
        assert b"qtos_probe: " in P.lib.qtos_last_error(P.h)
        assert all((got[k] == PATTERN).all() for k in OUT_F) and all((got[k] == IPATTERN).all() for k in OUT_I)
    for g, kw in [(ok(scale=7), {}), (ok(cols=0), {}), (ok(), dict(offsets=None)), (ok(), dict(slot=None)), (ok(), dict(status=None)),
                  (ok(), dict(bool_maps=None))]:
        rc, bm = stamp_device(gpu, maps.shape, g, T, status, **kw)
        assert rc == -2, (rc, kw)
        assert b"qtos_probe_stamp: " in P.lib.qtos_last_error(P.h)
        assert (bm.cpu().numpy() == PATTERN).all()
    with pytest.raises(RuntimeError):
        P.probe(maps, ok(scale=9))


# ---- the whole route on the golden map ----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def golden_route(gpu):
    """feasibility_map (host) and feasibility_maps_device on the golden map, once, on one handle."""
    from qtos_amd import feasibility, heightfield
    torch, dev, P, lp = gpu
    m = golden_map()
    lp.set_heightfield(heightfield.towr_map(m), heightfield.cell_size(m))
    bm, patches, statuses = feasibility.feasibility_map(lp, m, multi_map_shift=FIX["multi_map_shift"])
    out = feasibility.feasibility_maps_device(P, m, multi_map_shift=FIX["multi_map_shift"])
    torch.cuda.synchronize()
    return m, bm, patches, statuses, out


def test_device_route_is_the_host_route_on_the_golden_map(gpu, golden_route):
    torch = gpu[0]
    m, bm, patches, statuses, (d_bm, d_off, d_patch, d_status) = golden_route
    assert all(t.is_cuda for t in (d_bm, d_off, d_patch, d_status)) and d_bm.dtype == torch.float64 and tuple(d_bm.shape) == (1,) + m.shape
    got = d_status.cpu().numpy()
    print("statuses of the golden map's %d probes: %s" % (len(got), {int(k): int((got == k).sum()) for k in np.unique(got)}))
    assert d_off.cpu().tolist() == [0, 48] and len(patches) == 48
    assert d_patch.cpu().tolist() == [[0, p[2][0], p[2][1]] for p in patches]
    assert got.tolist() == [int(s) for s in statuses]
    assert np.array_equal(d_bm.cpu().numpy()[0], bm.astype(float))
    # a flat map has no problem and needs no solve
    from qtos_amd import feasibility
    flat = feasibility.feasibility_maps_device(gpu[2], torch.zeros((2, 6, 8), dtype=torch.float64, device=gpu[1]))
    assert flat[1].cpu().tolist() == [0, 0, 0] and not flat[0].any().item() and len(flat[2]) == 0 and len(flat[3]) == 0


def test_a_fleet_with_more_probes_than_max_batch_is_solved_in_chunks():
    """The chunk loop of feasibility_maps_device: 6 maps, about 90 probes, on a handle of 32 problems a call -- three calls on
    slices of the device arrays -- against feasibility_map per map on the same handle, one map's heightfield at a time."""
    import torch
    from qtos_amd import feasibility, heightfield
    from qtos_amd.planner import LocalPlanner
    maps = np.nan_to_num(gpu_batch(1))                                          # (heights the solver can stand on: the NaNs are flat ground)
    lp = LocalPlanner(max_batch=32)
    try:
        P = lp.planner()
        towr = np.stack([heightfield.towr_map(m) for m in maps])
        lp.set_heightfield(towr, 0.1)
        d_bm, d_off, d_patch, d_status = feasibility.feasibility_maps_device(P, maps, multi_map_shift=2)
        torch.cuda.synchronize()
        off, status, bm = d_off.cpu().numpy(), d_status.cpu().numpy(), d_bm.cpu().numpy()
        N = int(off[-1])
        assert N > 2 * 32 and len(status) == N and len(d_patch) == N
        print("%d probes in %d calls: statuses %s" % (N, -(-N // 32), {int(k): int((status == k).sum()) for k in np.unique(status)}))
        for k, m in enumerate(maps):
            lp.set_heightfield(towr[k], 0.1)
            want_bm, patches, statuses = feasibility.feasibility_map(lp, m, multi_map_shift=2)
            assert status[off[k]:off[k + 1]].tolist() == [int(v) for v in statuses], k
            assert d_patch.cpu().numpy()[off[k]:off[k + 1], 1:].tolist() == [list(p[2]) for p in patches]
            assert np.array_equal(bm[k], np.asarray(want_bm, float)), k
    finally:
        lp.close()


def test_the_tensor_goes_into_path_plan_and_repath(gpu, golden_route):
    from qtos_amd import capi, feasibility, heightfield, workloads
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import path_plan
    from qtos_amd.replan import ShiftedWindows
    torch, dev, P, _ = gpu
    m, bm, _, _, (d_bm, _, _, _) = golden_route
    NW = 4
    # a second map with obstacles whatever the solver answered: the stamp of the synthetic statuses, left on the device
    maps, shift, T, status = stamp_cases(1)[0]
    rc, d_syn = stamp_device(gpu, maps.shape, params(maps, shift, 1), T, status)
    assert rc == 0
    syn = feasibility.stamp_table(maps.shape, T["offsets"], T["slot"], T["patch"], status, 1)
    robot_goal = np.array([[4.5, 0.5, 0.24], [4.5, 0.0, 0.24], [2.5, 0.0, 0.24], [3.7, -0.6, 0.24]])
    start = np.stack([workloads.rest_start(0.02 * b, 0.01 * (b % 3 - 1), 0.24, np.zeros(4)) for b in range(NW)])
    par = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=0.6, max_cells=160, max_open=4096, max_pieces=80, set_done=True)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    host = lambda t: t.cpu().numpy().copy()
    for d_map, h_map in ((d_bm, bm[None].astype(float)), (d_syn, syn)):
        want = path_plan(h_map, None, start, robot_goal, par, done=np.zeros(NW, np.int32))
        # straight into qtos_path_plan_device
        g = capi.path_plan_params(step_size=0.6, max_cells=160, max_pieces=80, set_done=True, bool_map=h_map)
        D = dict(start=torch.as_tensor(start, **f64), rg=torch.as_tensor(robot_goal, **f64), knots=torch.zeros((NW, 81), **f64),
                 coef=torch.zeros((NW, 2, 4, 80), **f64), n=torch.zeros((NW,), **i32), cells=torch.zeros((NW, 160, 2), **i32),
                 nc=torch.zeros((NW,), **i32), st=torch.zeros((NW,), **i32), done=torch.zeros((NW,), **i32))
        rc = P.lib.qtos_path_plan_device(P.h, NW, C.byref(g), d_map.data_ptr(), None, *[D[k].data_ptr() for k in
                                         ("start", "rg", "knots", "coef", "n", "cells", "nc", "st", "done")],
                                         C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, P.lib.qtos_last_error(P.h)
        print("paths over the map: status %s cells %s" % (host(D["st"]).tolist(), host(D["nc"]).tolist()))
        assert np.array_equal(host(D["st"]), want["status"]) and np.array_equal(host(D["cells"]), want["cells"])
        assert same(host(D["knots"]), want["knots"]) and same(host(D["coef"]), want["coef"])
    assert syn.sum() > 0
    # and into a set of windows: the tensor on the set's stream, against the numpy form over the same map
    W = capi.Planner(PlannerConfig.receding_windows(), max_batch=NW)
    try:
        W.set_heightfields(heightfield.towr_map(m)[None], 0.1)
        plan = dict(bool_map=np.zeros_like(syn), robot_goal=robot_goal, max_pieces=80)
        S = ShiftedWindows(W, start, None, np.zeros(NW, np.int32), advance=3.0, path=dict(plan=plan, map_yx=m, step_size=0.6))
        tables = []
        for form in (d_syn, syn, d_bm):
            S.repath(bool_map=form)
            torch.cuda.synchronize()
            tables.append(dict(knots=host(S._path_knots), coef=host(S._path_coef), n=host(S._path_n), cells=host(S.path_cells),
                               status=host(S.path_status), maps=host(S._plan_maps)))
        want = path_plan(syn, None, start, robot_goal, par, done=np.zeros(NW, np.int32))
        for t in tables[:2]:
            assert same(t["maps"], syn) and np.array_equal(t["cells"], want["cells"]) and np.array_equal(t["status"], want["status"])
            assert same(t["knots"], want["knots"]) and same(t["coef"], want["coef"]) and np.array_equal(t["n"], want["n_pieces"])
        assert same(tables[2]["maps"], bm[None].astype(float))
        # a set with a stream of its own, the tensor made on another one and dropped at once: the copy on the set's stream, held up
        # behind other work, still reads the map, not what the caller's next allocation on its stream puts into the block
        own, side = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
        S2 = ShiftedWindows(W, start, None, np.zeros(NW, np.int32), advance=3.0, stream=own, path=dict(plan=plan, map_yx=m, step_size=0.6))
        busy = torch.ones((2048, 2048), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        with torch.cuda.stream(own):
            for _ in range(20):
                busy = (busy @ busy).clamp_(0.0, 1.0)
        with torch.cuda.stream(side):
            t = torch.as_tensor(syn, **f64) + 0.0
            S2.repath(bool_map=t)
            del t
            junk = [torch.zeros(syn.shape, **f64) for _ in range(4)]
        torch.cuda.synchronize()
        assert same(host(S2._plan_maps), syn) and len(junk) == 4
        assert np.array_equal(host(S2.path_cells), want["cells"]) and np.array_equal(host(S2.path_status), want["status"])
        assert same(host(S2._path_knots), want["knots"]) and same(host(S2._path_coef), want["coef"])
        with torch.cuda.stream(own):                                            # (made on the set's own stream: no wait is needed)
            S2.repath(bool_map=torch.as_tensor(bm[None].astype(float), **f64))
        torch.cuda.synchronize()
        assert same(host(S2._plan_maps), bm[None].astype(float))
        with pytest.raises(ValueError):
            S.repath(bool_map=d_syn[:, :10])
        with pytest.raises(ValueError):
            S.repath(bool_map=d_syn.to(torch.float32))
    finally:
        W.close()


def test_c_caller_probes_solves_stamps_and_plans(tmp_path):
    from qtos_amd import capi, feasibility
    from qtos_amd.config import PlannerConfig
    from qtos_amd.global_planner import path_plan
    capi.load()
    exe = tmp_path / "probe_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "probe_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.reference_compat())))
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img)], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout[:2000], r.stderr)
    lines = r.stdout.splitlines()
    assert lines[0] == "sizeof_probe=%d probe_null=-1 probe_device_null=-1 probe_stamp_null=-1" % C.sizeof(capi.QtosProbe)
    assert lines[1] == "bad_args=-2,-2,-2,-2,-2,-2 untouched=1 reason=1"
    m = np.zeros((20, 20))
    m[10, 10] = 0.05
    T = feasibility.probe_table(m)
    N = len(T["patch"])
    toks = lines[2].split()
    assert toks[0:2] == ["probe=0", "n=%d" % N] and N == 4
    status = []
    for i, t in enumerate(toks[2:]):
        v = t.split("=")[1].split(",")
        assert [int(x) for x in v[0:3]] == T["patch"][i].tolist()
        status.append(int(v[3]))
        assert same(np.array([float(x) for x in v[4:7]]), T["start"][i, 0:3]) and same(np.array([float(x) for x in v[7:10]]), T["goal"][i])
    bm = feasibility.stamp_table(m.shape, T["offsets"], T["slot"], T["patch"], np.array(status), 1)
    assert lines[3] == "bool_map=" + "".join(str(int(v)) for v in bm.ravel())
    start = np.zeros((1, 24))
    start[0, 0:3] = [-0.85, 0.05, 0.24]
    par = dict(cell=0.1, origin_x=1.0, origin_y=1.0, height_bound=0.2, step_size=0.25, max_cells=80, max_open=1024, max_pieces=40, set_done=False)
    want = path_plan(bm, None, start, np.array([[0.85, 0.05, 0.24]]), par)
    q = dict(t.split("=") for t in lines[4].split())
    assert (int(q["path_plan"]), int(q["status"]), int(q["n_cells"]), int(q["n_pieces"])) == (0, want["status"][0], want["n_cells"][0], want["n_pieces"][0])
    assert [int(v) for v in q["cells"].split(",")] == want["cells"][0].ravel().tolist() and want["status"][0] == 0
