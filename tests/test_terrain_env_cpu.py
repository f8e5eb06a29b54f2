"""The randomised terrain without a GPU: heightfield.random_env (the reference's four calls on a `random.Random`) and
heightfield.random_env_table (the statement in arrays and integers that k_terrain_env equals) against the reference's own maps
(tests/golden/random_env.json, written by tests/golden/make_random_env_golden.py) to the bit, the stream position behind them,
the from-scratch MT19937 against `random.Random`, the merge of two levels, the statuses, the ABI and the kernel's resources in
the gfx950 code object.  The GPU tests (tests/test_gpu_terrain_env.py) import the cases from here."""
import ctypes as C
import hashlib
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

FIX = json.load(open(os.path.join(GOLDEN, "random_env.json")))
CASES = FIX["cases"]
case_id = lambda c: "%s-x%d-seed%d" % (c["base"], c["mesh_scale"], c["seed"])


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(bits(a), bits(b))


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def case_base(c):
    from qtos_amd import heightfield
    return heightfield.scale_map(np.array(FIX["bases"][c["base"]]["map"], dtype=float), c["mesh_scale"])


def synthetic_batch():
    """Six 7 x 10 maps: flat, one level, eight levels, negative levels and -0.0, 65 levels (status 1), one NaN (status 3)."""
    rng = np.random.default_rng(11)
    maps = np.zeros((6, 7, 10))
    maps[1, 2:5, 3:7] = 0.3
    maps[2] = rng.choice(np.array([0.0, 0.05, 0.1, 0.15, 0.2, 0.25, 0.3, 0.35, 0.4]), size=(7, 10))
    maps[3] = rng.choice(np.array([0.0, -0.0, -0.1, -0.004, 0.003, 0.2]), size=(7, 10))
    maps[3, 0, 0], maps[3, 6, 9] = -0.0, -0.1
    maps[4] = (np.arange(70).reshape(7, 10) % 66) * 0.01              # 0 and 65 levels
    maps[5] = maps[2]
    maps[5, 3, 4] = np.nan
    assert len(np.unique(maps[2][maps[2] != 0])) == 8 and len(np.unique(maps[4][maps[4] != 0])) == 65
    assert np.signbit(maps[3][maps[3] == 0]).any()
    return maps, [5, 6, 2**32 + 7, 8, 9, 10]


def table(c, **kw):
    from qtos_amd import heightfield
    return heightfield.random_env_table(case_base(c), [c["seed"]], n_shift=c["n_shift"], n_height=FIX["n_height"], climb=c["climb"],
                                        delta=FIX["delta"], **kw)


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_random_env_is_the_reference_map_and_leaves_its_stream(c):
    from qtos_amd import heightfield
    rng = random.Random(c["seed"])
    m = heightfield.random_env(case_base(c), rng, c["n_shift"], FIX["n_height"], c["climb"])
    assert sha(m) == c["sha256"]
    assert rng.getrandbits(32) == c["next_bits"]
    if "map" in c:
        assert same(m, np.array(c["map"]))
    assert [float(v) for v in np.unique(m[m != 0])] == c["levels"]


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_table_is_the_reference_map_and_leaves_its_stream(c):
    from qtos_amd import heightfield
    T = table(c)
    assert T["status"].tolist() == [0]
    assert sha(T["map_yx"][0]) == c["sha256"] and T["net_shift"][0].tolist() == c["net_shift"]
    assert same(T["height_xy"][0], heightfield.towr_map(T["map_yx"][0]))
    assert heightfield.MT19937(c["seed"], int(T["draws"][0])).bits32() == c["next_bits"]
    if c["base"] == "exp_5":                               # the climb map crosses a regeneration of the 624-word state
        assert T["draws"][0] > 624


def test_table_batches_fan_out_and_carry_draws():
    from qtos_amd import heightfield
    cs = [c for c in CASES if c["base"] == "exp_3" and c["mesh_scale"] == 1]
    base = np.stack([case_base(cs[0]), case_base(cs[0])[::-1].copy()])
    T = heightfield.random_env_table(base, [c["seed"] for c in cs], base_id=[0] * len(cs))
    for k, c in enumerate(cs):
        assert sha(T["map_yx"][k]) == c["sha256"]
    # two calls that carry draws are one stream: update() twice behind the constructor's sequence
    U = FIX["update"]
    T = heightfield.random_env_table(np.array(FIX["bases"][U["base"]]["map"]), [U["seed"]], n_shift=U["n_shift"])
    m, draws = T["map_yx"], T["draws"]
    for step in U["steps"]:
        T = heightfield.random_env_table(m, [U["seed"]], draws=draws, n_shift=1, n_height=0)
        m, draws = T["map_yx"], T["draws"]
        assert same(m[0], np.array(step["map"]))
    assert heightfield.MT19937(U["seed"], int(draws[0])).bits32() == U["next_bits"]


@pytest.mark.parametrize("seed", [0, 1, 12345, 2**32 - 1, 2**32, 2**32 + 5, 2**64 - 1])
def test_mt19937_is_pythons(seed):
    from qtos_amd import heightfield
    r, m = random.Random(seed), heightfield.MT19937(seed)
    assert [m.bits32() for _ in range(2000)] == [r.getrandbits(32) for _ in range(2000)]
    r, m = random.Random(seed), heightfield.MT19937(seed)
    for _ in range(300):
        assert bits(m.uniform(-0.005, 0.005)) == bits(r.uniform(-0.005, 0.005))
        assert m.below(3) == r.choice((0, 1, 2)) and m.below(4) == r.choice((0, 1, 2, 3)) and m.below(2) == r.choice((0, 1))
    r = random.Random(seed)
    want = [r.getrandbits(32) for _ in range(1900)]
    for skip in (0, 1, 623, 624, 625, 1247, 1248, 1899):
        m = heightfield.MT19937(seed, skip)
        assert m.bits32() == want[skip] and m.draws == skip + 1


def test_levels_that_collide_merge_and_draw_less():
    from qtos_amd import heightfield
    M = FIX["merge"]
    out = {}
    for k in ("separate", "merged"):
        base = np.array(M[k]["base"])
        rng = random.Random(M["seed"])
        assert same(heightfield.random_env(base, rng, 0, FIX["n_height"]), np.array(M[k]["map"]))
        assert rng.getrandbits(32) == M[k]["next_bits"]
        T = heightfield.random_env_table(base, [M["seed"]], n_shift=0)
        assert same(T["map_yx"][0], np.array(M[k]["map"]))
        assert heightfield.MT19937(M["seed"], int(T["draws"][0])).bits32() == M[k]["next_bits"]
        out[k] = T
    levels = lambda a: np.unique(a[a != 0])
    assert len(levels(np.array(M["merged"]["base"]))) == 2
    assert len(levels(out["merged"]["map_yx"][0])) == 1 and len(levels(out["separate"]["map_yx"][0])) == 2
    assert out["merged"]["draws"][0] < out["separate"]["draws"][0]


def test_random_map_shift_is_the_reference():
    from qtos_amd import heightfield
    for c in FIX["map_shift"]:
        rng = random.Random(c["seed"])
        m = heightfield.random_map_shift(np.array(FIX["bases"][c["base"]]["map"]), c["shift"], rng, c["climb"])
        assert same(m, np.array(c["map"])) and rng.getrandbits(32) == c["next_bits"]


def test_statuses():
    from qtos_amd import heightfield
    maps, seeds = synthetic_batch()
    T = heightfield.random_env_table(maps, seeds, fill=-7.0)
    assert T["status"].tolist() == [0, 0, 0, 0, 1, 3]
    assert same(T["map_yx"][0], np.zeros((7, 10))) and T["draws"][0] >= 20      # a flat map: the shifts alone draw
    for k in (4, 5):
        assert (T["map_yx"][k] == -7.0).all() and (T["height_xy"][k] == -7.0).all() and T["draws"][k] == 0
    assert np.signbit(T["map_yx"][3][T["map_yx"][3] == 0]).any()                 # -0.0 is ground, and stays -0.0
    assert len(np.unique(T["map_yx"][3][T["map_yx"][3] != 0])) <= 4
    draws = np.array([0, 2**24, 2**24 + 1, -1, 5, 5], np.int32)
    T = heightfield.random_env_table(maps, seeds, draws=draws, n_shift=1, n_height=0, fill=-7.0)
    assert T["status"].tolist() == [0, 0, 2, 2, 1, 3] and T["draws"][2:].tolist() == [2**24 + 1, -1, 5, 5]
    assert 2 <= T["draws"][0] < 20 and 2 <= T["draws"][1] - 2**24 < 20
    maps[2, 0, 0] = np.nan
    assert heightfield.random_env_table(maps[2:3], [1], draws=[2**24 + 1])["status"].tolist() == [2]
    both = maps[4].copy()
    both[0, 0] = np.nan
    assert heightfield.random_env_table(both, [1])["status"].tolist() == [3]
    # a base_id that names no base grid: status 4, behind the draws' check and in front of the grid's
    T = heightfield.random_env_table(maps, [1, 2, 3, 4], base_id=[0, 6, -1, 7], draws=[0, 0, 0, 2**24 + 1], fill=-7.0)
    assert T["status"].tolist() == [0, 4, 4, 2] and (T["map_yx"][1:] == -7.0).all() and T["draws"][1:].tolist() == [0, 0, 2**24 + 1]


def test_workload_is_random_env_per_map():
    from qtos_amd import heightfield, workloads
    maps, height_xy, cell = workloads.random_env_terrains(3, seed=0, tiles=("climb_2", "climb_1"), mesh_scale=1)
    for m, seed in zip(maps, (0, 1, 2)):
        c = [c for c in CASES if c["base"] == "exp_5" and c["seed"] == seed][0]
        assert sha(m) == c["sha256"]
    assert same(height_xy[1], heightfield.towr_map(maps[1])) and cell == 0.1


def test_abi_exports_and_layout(hip_lib):
    from qtos_amd import capi
    for name in ("qtos_terrain_env", "qtos_terrain_env_device", "qtos_set_heightfields_device"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    g = capi.QtosTerrainEnv
    assert [f[0] for f in g._fields_] == ["n_maps", "n_base", "rows", "cols", "n_shift", "n_height", "climb", "delta"]
    assert C.sizeof(g) == 40 and g.delta.offset == 32 and g.climb.offset == 24
    p = capi.terrain_env_params(np.zeros((3, 7, 10)), n_maps=16, n_shift=20, climb=True)
    assert (p.n_maps, p.n_base, p.rows, p.cols, p.n_shift, p.n_height, p.climb, p.delta) == (16, 3, 7, 10, 20, 10, 1, 0.005)
    header = open(os.path.join(ROOT, "include", "qtos_planner.h")).read()
    assert int(re.search(r"#define QTOS_ENV_MAX_LEVELS (\d+)", header).group(1)) == capi.ENV_MAX_LEVELS
    assert int(re.search(r"#define QTOS_ENV_LDS_BYTES (\d+)", header).group(1)) == capi.ENV_LDS_BYTES
    from qtos_amd import heightfield
    assert (heightfield.ENV_MAX_LEVELS, heightfield.ENV_MAX_DRAWS) == (capi.ENV_MAX_LEVELS, capi.ENV_MAX_DRAWS)


def test_kernel_uses_no_scratch_and_the_lds_of_the_header(hip_lib, tmp_path):
    from qtos_amd import capi
    llvm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "k.co")
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, capi.LIB_PATH])
    subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], text=True)
    blocks = [b for b in text.split("- .agpr_count")[1:] if re.search(r"\.name:\s+\S*k_terrain_env", b)]
    assert len(blocks) == 1
    field = lambda name: int(re.search(r"\.%s:\s+(\d+)" % name, blocks[0]).group(1))
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    assert field("group_segment_fixed_size") == capi.ENV_LDS_BYTES
    assert field("max_flat_workgroup_size") == 256
    # the draws round product and sum one by one: no fused multiply-add anywhere in the kernel's code
    name = re.search(r"\.name:\s+(\S*k_terrain_env\S*)", blocks[0]).group(1)
    code = subprocess.check_output([os.path.join(llvm, "llvm-objdump"), "-d", "--disassemble-symbols=" + name, co], text=True)
    ops = re.findall(r"^\s+(v_\w+)", code, re.M)
    assert len(ops) > 200 and any(o.startswith("v_add_f64") for o in ops) and any(o.startswith("v_mul_f64") for o in ops)
    assert not [o for o in ops if "fma" in o or "mad_f" in o or "mac_f" in o]
