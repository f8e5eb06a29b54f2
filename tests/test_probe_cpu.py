"""The probe and the stamp of the windows' heightfields without a GPU: the array statement of k_probe / k_probe_stamp
(feasibility.probe_table, round2, stamp_table) against the host route that is pinned to the reference (probe_patches, patch_args,
stamp and the fixture planner.json["path_map"]), the C ABI of qtos_probe*, and the resources of the kernels read from the gfx950
code object.  The batches of maps and the synthetic statuses that the GPU test runs (tests/test_gpu_probe.py) are built here."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from test_path_goal_cpu import bits, same  # noqa: E402
from test_stitch_cpu import CSRC, field, notes, one_kernel  # noqa: E402,F401  (the code object's notes, read as that file reads them)

GOLDEN = os.path.join(ROOT, "tests", "golden")
FIX = json.load(open(os.path.join(GOLDEN, "planner.json")))["path_map"]
SHAPES = ((2, 3), (3, 4), (5, 8), (7, 9), (20, 20))
STAMP_SEED = 5


def tile(name):
    from qtos_amd import heightfield
    return heightfield.read_tile(os.path.join(GOLDEN, "heightfields", name + ".txt"))


def golden_map():
    from qtos_amd import heightfield
    return heightfield.build_map([tile(t) for t in FIX["tiles"]], 1)


def random_map(rng, shape, kind):
    """One seeded map: "inner" obstacles off the border, "border" positive cells on it (the early False of the danger test),
    "negative" and "nan" heights among the obstacles, "zero" the flat ground."""
    rows, cols = shape
    m = np.zeros(shape)
    if kind == "zero":
        return m
    hit = rng.random(shape) < 0.12
    m[hit] = np.round(rng.uniform(0.02, 0.3, int(hit.sum())), 3)
    if kind == "inner":
        m[0, :] = m[-1, :] = 0.0
        m[:, 0] = m[:, -1] = 0.0
    if kind == "border":
        m[0, :] = np.where(rng.random(cols) < 0.5, 0.1, m[0, :])
        m[:, -1] = np.where(rng.random(rows) < 0.5, 0.07, m[:, -1])
    if kind == "negative":
        neg = rng.random(shape) < 0.15
        m[neg] = -np.round(rng.uniform(0.0, 0.2, int(neg.sum())), 3)      # (-0.0 among them)
    if kind == "nan":
        m[rng.random(shape) < 0.15] = np.nan
    return m


KINDS = ("inner", "border", "negative", "nan", "zero")


def gpu_batch(scale):
    """The batch of 6 maps of 7 x 10 the GPU test probes: every kind of map, and a dense one."""
    rng = np.random.default_rng(100 + scale)
    maps = [random_map(rng, (7, 10), k) for k in KINDS]
    dense = np.round(rng.uniform(-0.05, 0.2, (7, 10)), 3)
    return np.stack(maps + [dense])


def host_patches(maps, shift, scale):
    from qtos_amd import feasibility
    return [feasibility.probe_patches(m, shift, 0.1 * (1 / scale)) for m in maps]


def assert_table_is_probe_patches(maps, shift, scale):
    """probe_table against probe_patches (coordinates and indices) and flags.problem_arrays(patch_args) (start, goal), to the bit."""
    from qtos_amd import feasibility, flags
    maps = np.asarray(maps, float)
    maps = maps[None] if maps.ndim == 2 else maps
    T = feasibility.probe_table(maps, shift, scale)
    per_map = host_patches(maps, shift, scale)
    n_maps, rows, cols = maps.shape
    assert T["offsets"].dtype == T["slot"].dtype == T["patch"].dtype == T["map_id"].dtype == np.int32
    assert T["offsets"].tolist() == np.concatenate([[0], np.cumsum([len(p) for p in per_map])]).tolist()
    N = int(T["offsets"][-1])
    assert T["slot"].shape == (n_maps, rows, cols // 2 - 1) and T["patch"].shape == (N, 3)
    assert T["start"].shape == (N, 24) and T["goal"].shape == (N, 3) and T["map_id"].shape == (N,)
    slot = np.full(T["slot"].shape, -1, np.int32)
    i = 0
    for m, patches in enumerate(per_map):
        for s_pt, g_pt, s_idx, g_idx in patches:
            assert T["patch"][i].tolist() == [m, s_idx[0], s_idx[1]] and g_idx == (s_idx[0], s_idx[1] + 2) and T["map_id"][i] == m
            start, goal, _ = flags.problem_arrays(feasibility.patch_args(s_pt, g_pt))
            assert same(T["start"][i], np.array(start)), (m, s_idx, T["start"][i], start)
            assert same(T["goal"][i], np.array(goal)), (m, s_idx, T["goal"][i], goal)
            assert same(T["start"][i, 0:2], np.array(s_pt[0:2])) and same(T["goal"][i, 0:2], np.array(g_pt[0:2]))
            slot[m, s_idx[0], s_idx[1] // 2] = i
            i += 1
    assert i == N and np.array_equal(T["slot"], slot)
    return T


def test_probe_table_is_the_golden_fixture():
    m = golden_map()
    assert m.shape == (20, 60)
    T = assert_table_is_probe_patches(m, FIX["multi_map_shift"], 1)
    assert len(FIX["patches"]) == 48 == len(T["patch"])
    for i, r in enumerate(FIX["patches"]):
        z, zg = m[tuple(r[2])], m[tuple(r[3])]
        assert T["patch"][i].tolist() == [0] + r[2] and r[3] == [r[2][0], r[2][1] + 2]
        assert same(T["start"][i, 0:3], np.array([r[0][0], r[0][1], z + 0.24])) and float(z) == r[0][2]
        assert same(T["goal"][i], np.array([r[1][0], r[1][1], zg + 0.24])) and float(zg) == r[1][2]


@pytest.mark.parametrize("name", FIX["tiles"])
def test_probe_table_on_each_golden_tile(name):
    from qtos_amd import heightfield
    for shift in (1, 2, 3):
        assert_table_is_probe_patches(heightfield.build_map([tile(name)], 1), shift, 1)


@pytest.mark.parametrize("scale", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_probe_table_on_seeded_maps(shape, scale):
    rng = np.random.default_rng(1000 * shape[0] + 10 * shape[1] + scale)
    total = 0
    for shift in (1, 2, 3):
        maps = np.stack([random_map(rng, shape, k) for k in KINDS])
        T = assert_table_is_probe_patches(maps, shift, scale)
        total += len(T["patch"])
        assert T["offsets"][-1] == T["offsets"][-2], "the all-zero map has no patch"
    assert (total == 0) == (shape == (2, 3)), total


@pytest.mark.parametrize("scale", [1, 2])
def test_the_gpu_batches_hold_the_cases(scale):
    maps = gpu_batch(scale)
    T = assert_table_is_probe_patches(maps, 2, scale)
    n = np.diff(T["offsets"])
    assert n[4] == 0 and (n[[0, 1, 2, 3, 5]] > 0).all() and np.isnan(maps[3]).any() and (maps[2] < 0).any()
    assert (T["slot"] == -1).any() and np.isnan(T["start"]).any() == bool(np.isnan(maps[T["patch"][:, 0], T["patch"][:, 1], T["patch"][:, 2]]).any())


def test_round2_is_pythons_round():
    from qtos_amd import feasibility
    rng = np.random.default_rng(7)
    parts = [rng.uniform(-50, 50, 40000),
             np.round(rng.uniform(-30, 30, 30000), 3),                               # three decimals: the ...5 coordinates of fine cells
             rng.integers(-4000, 4000, 20000) / 8.0 / 100.0 * 4.0 + 0.005,           # near ties
             (2 * rng.integers(-20000, 20000, 20000) + 1) / 200.0,                   # k + 0.5 hundredths as doubles: ties up to rounding
             (2 * rng.integers(-4000, 4000, 10000) + 1) / 8.0]                       # x.125, x.375, ...: exact ties
    v = np.concatenate(parts)
    assert len(v) >= 100000
    want = np.array([round(float(x), 2) for x in v])
    got = feasibility.round2(v)
    assert same(got, want), np.argwhere(bits(got) != bits(want))[:5].tolist()
    p = v * 100.0
    ties = int((np.abs(p - np.rint(p)) == 0.5).sum())
    from fractions import Fraction
    half = v[np.abs(p - np.rint(p)) == 0.5]
    exact = sum(1 for x in half if (Fraction(float(x)) * 200).denominator == 1)      # v * 100 is k + 1/2 in exact arithmetic
    print("round2: %d values, %d ties of the rounded product, %d of them exact ties" % (len(v), ties, exact))
    assert ties >= 1000 and exact >= 1000 and ties - exact >= 1000
    naive = np.rint(p) / 100.0
    assert not same(naive, want), "the cases hold values on which rint(v * 100) / 100 is not round(v, 2)"
    assert feasibility.round2(0.125) == round(0.125, 2) and isinstance(feasibility.round2(2.675), float)
    assert feasibility.round2(2.675) == round(2.675, 2) == 2.67 and feasibility.round2(1.005) == round(1.005, 2)


def synthetic_statuses(n, seed=STAMP_SEED):
    """Statuses drawn from {0, 1, 2}: alternating on the first half (a success clears what a failure wrote and the reverse),
    seeded on the rest."""
    rng = np.random.default_rng(seed)
    st = rng.integers(0, 3, n).astype(np.int32)
    st[:n // 2:2] = 0
    st[1:n // 2:2] = 1 + (np.arange(len(st[1:n // 2:2])) % 2)
    return st


def stamp_cases(scale):
    """(maps, shift, table, statuses) of the stamp tests: the golden map at scale 1, the GPU batch at the given scale."""
    from qtos_amd import feasibility
    out = []
    for maps, shift in ((golden_map()[None], FIX["multi_map_shift"]), (gpu_batch(scale), 2)):
        T = feasibility.probe_table(maps, shift, scale)
        out.append((maps, shift, T, synthetic_statuses(len(T["patch"]))))
    return out


def overwrites(shape, patches, statuses, scale):
    """(cells a success cleared after a failure wrote them, cells a failure wrote after a success cleared them) of one map."""
    from qtos_amd import feasibility
    wrote = np.full(shape, -1)
    cleared = flipped = 0
    for k in range(len(patches)):
        before = feasibility.stamp(shape, patches[:k], statuses[:k], scale)
        after = feasibility.stamp(shape, patches[:k + 1], statuses[:k + 1], scale)
        s = patches[k][2]
        if statuses[k] == 0:
            for c in ((s[0], s[1]), (s[0], s[1] + 1), (s[0], s[1] + 2)):
                cleared += int(before[c] == 1)
                wrote[c] = 0
        else:
            flipped += int(((wrote == 0) & (after == 1)).sum())
            wrote[after == 1] = np.where(wrote[after == 1] == 0, 1, wrote[after == 1])
    return cleared, flipped


@pytest.mark.parametrize("scale", [1, 2])
def test_stamp_table_is_stamp_per_map(scale):
    from qtos_amd import feasibility
    cleared = flipped = 0
    for maps, shift, T, st in stamp_cases(scale):
        assert set(st.tolist()) == {0, 1, 2}
        got = feasibility.stamp_table(maps.shape, T["offsets"], T["slot"], T["patch"], st, scale)
        assert got.dtype == np.float64 and got.shape == maps.shape and set(np.unique(got)) <= {0.0, 1.0}
        per_map = host_patches(maps, shift, scale)
        for m, patches in enumerate(per_map):
            s = st[T["offsets"][m]:T["offsets"][m + 1]].tolist()
            want = feasibility.stamp(maps[m].shape, patches, s, scale)
            assert np.array_equal(got[m], want.astype(float)), (m, np.argwhere(got[m] != want)[:5].tolist())
            a, b = overwrites(maps[m].shape, patches, s, scale)
            cleared, flipped = cleared + a, flipped + b
        assert same(feasibility.stamp_table(maps.shape[1:], T["offsets"], T["slot"], T["patch"], st, scale), got)
    print("stamp, scale %d: %d cells cleared by a success after a failure, %d written by a failure after a success" % (scale, cleared, flipped))
    assert cleared >= 1 and flipped >= 1


def test_abi_exports_and_struct_size(tmp_path):
    from qtos_amd import capi
    lib = capi.load()
    names = ("qtos_probe", "qtos_probe_device", "qtos_probe_stamp", "qtos_probe_stamp_device")
    assert all(n in capi.EXPORTS and hasattr(lib, n) for n in names)
    fields = [f for f, _ in capi.QtosProbe._fields_]
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qtos_planner.h"\nint main(void) { printf("%d", (int)sizeof(QtosProbe));\n'
                   + "".join('printf(" %%d", (int)offsetof(QtosProbe, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.QtosProbe
    assert got == [C.sizeof(S)] + [getattr(S, f).offset for f in fields]
    g = capi.probe_params(np.zeros((3, 7, 10)), multi_map_shift=2, scale=2)
    assert (g.n_maps, g.rows, g.cols, g.scale, g.multi_map_shift, g.cell, g.origin_shift, g.z_offset) == (3, 7, 10, 2, 2, 0.1, 1.0, 0.24)
    nested = capi.probe_params([[0.0] * 10] * 7)                                # (a map as a list of rows; a shape; a tensor-like)
    assert (nested.n_maps, nested.rows, nested.cols) == (1, 7, 10) == tuple(getattr(capi.probe_params((7, 10)), k) for k in ("n_maps", "rows", "cols"))
    assert (capi.probe_params([3, 7, 10]).n_maps, capi.probe_params(np.zeros((2, 3))).cols) == (3, 3)
    with pytest.raises(ValueError):
        capi.probe_params(np.zeros(5))
    from qtos_amd.feasibility import NOMINAL_STANCE
    assert [list(r) for r in g.nominal_stance] == [list(r) for r in NOMINAL_STANCE]
    # the argument checks that need no planner
    assert lib.qtos_probe_device(None, C.byref(g), None, 0, None, None, None, None, None, None, None) == -1
    assert lib.qtos_probe_stamp_device(None, C.byref(g), None, None, None, None, None, None) == -1
    assert lib.qtos_probe(None, C.byref(g), None, 0, None, None, None, None, None, None) == -1
    assert lib.qtos_probe_stamp(None, C.byref(g), None, None, None, None, None) == -1


def test_c99_probe_caller_builds_and_checks_its_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "probe_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "probe_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.reference_compat())))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_probe"]) == C.sizeof(capi.QtosProbe)
    assert int(kv["probe_null"]) == -1 and int(kv["probe_stamp_null"]) == -1


# (static LDS: k_probe's coordinates are dynamic LDS, rows + cols / 2 + 12 doubles, sized at the launch)
@pytest.mark.parametrize("kernel,lds", [("k_probe_count", 0), ("k_probe_scan", 256 * 4), ("k_probe", 0), ("k_probe_stamp", 0)])
def test_probe_kernels_use_no_scratch(notes, kernel, lds):  # noqa: F811
    block = one_kernel(notes, kernel)
    assert field(block, "private_segment_fixed_size") == 0, "scratch bytes per lane"
    assert field(block, "vgpr_spill_count") == 0 and field(block, "sgpr_spill_count") == 0
    assert field(block, "group_segment_fixed_size") == lds
