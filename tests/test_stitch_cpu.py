"""Stitching of receding windows without a GPU: the numpy statement of k_stitch's rule (stitcher.stitch_segments, ring_append)
against the host Stitcher, which is pinned to the reference, the C ABI of qtos_stitch*, the C99 loop's build and argument checks,
and the resources of k_stitch / k_sample read from the gfx950 code object."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LIB = os.path.join(CSRC, "libqtos_planner.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")

HZ = 1000
N_PLAN = 5001
HANDOVER = (2500, 2757, 2613)      # the hand-over row of plans 0, 1 (and of plan 2, not used: the loop ends there)


def synthetic_plans():
    """Three plans' tables: 37 columns, a value that names plan, row and column in every cell but the feet's z (columns 9, 12,
    15, 18), which is 0 -- the height rule passes at the first candidate; time stamps chained by the hand-over rows."""
    tables, t0 = [], 0.0
    for i in range(3):
        k = np.arange(N_PLAN)
        t = (i + 1) * 1e6 + k[:, None] * 100.0 + np.arange(37)[None, :]
        t[:, 0] = t0 + k / HZ
        t[:, [9, 12, 15, 18]] = 0.0
        tables.append(t)
        t0 = t0 + HANDOVER[i] / HZ
    return tables


@pytest.mark.parametrize("mode,first_row", [("clean", 0), ("reference", 1)])
def test_segments_are_what_the_stitcher_chain_keeps(mode, first_row):
    from qtos_amd.stitcher import Stitcher, stitch_segments
    tables = synthetic_plans()
    st = Stitcher(lookahead=HANDOVER[0], hz=HZ, height_set=(0.0,), mode=mode)
    executed, rows, last = [], [], None
    for i in range(2):                                  # plan i is executing, plan i + 1 takes over
        st.lookahead_original = HANDOVER[i]
        st.cutoff_idx = 0
        st.state(tables[i], tables[i][0, 0])             # the hand-over row of plan i, searched from its own first row
        r = st.next_traj_step
        assert r == st.lookahead == HANDOVER[i]          # (all feet at z = 0: the first candidate)
        assert tables[i + 1][0, 0] == tables[i][0, 0] + r / HZ
        rows.append(r)
        last = st.combine(tables[i], tables[i + 1])      # old up to the hand-over ++ new
        if i == 0:
            executed.append(last[:r])                    # what plan 0 contributed before plan 1 took over
    chain = np.concatenate(executed + [last], axis=0)
    want = np.concatenate([stitch_segments(tables[:2], rows, first_row), tables[2][first_row:]], axis=0)
    assert chain.shape == want.shape == (sum(rows) + N_PLAN - first_row, 37)
    assert np.array_equal(chain, want)
    # the segments by hand
    assert np.array_equal(want[:rows[0]], tables[0][first_row:first_row + rows[0]])
    assert np.array_equal(want[rows[0]:rows[0] + rows[1]], tables[1][first_row:first_row + rows[1]])
    if mode == "clean":
        # every row once: the time stamps go on by 1 / hz across the splices
        assert np.allclose(np.diff(want[:, 0]), 1.0 / HZ, rtol=0, atol=1e-9)
        # and the chain through ONE growing file (the stitched file is the old file of the next combine) gives the same rows
        st2 = Stitcher(lookahead=HANDOVER[0], hz=HZ, height_set=(0.0,), mode="clean")
        grown = tables[0]
        for i in range(2):
            st2.lookahead_original = HANDOVER[i]
            st2.cutoff_idx = 0
            st2.state(grown, tables[i][0, 0])
            grown = st2.combine(grown, tables[i + 1])
        assert np.array_equal(grown, want)
    else:
        # the reference's file: the old plan's hand-over row stays and the new plan starts at its second row
        assert want[rows[0] - 1, 0] == tables[0][rows[0], 0] and want[rows[0], 0] == tables[1][1, 0]
    with pytest.raises(ValueError):
        stitch_segments(tables[:1], [N_PLAN], 1)


def test_ring_append_is_concatenate_and_slice():
    from qtos_amd.stitcher import ring_append, ring_rows
    cap = 300
    rng = np.random.default_rng(3)
    ring = np.full((cap, 37), -7.0)
    everything = np.zeros((0, 37))
    cursor = 0
    for n in (0, 1, 200, 257, 300, 120, 0, 5):          # 883 rows in all: the cursor wraps twice
        seg = rng.standard_normal((n, 37))
        new = ring_append(ring, cursor, seg)
        assert new == cursor + n
        cursor = new
        everything = np.concatenate([everything, seg], axis=0)
        valid = min(cursor, cap)
        assert np.array_equal(ring_rows(ring, cursor), everything[len(everything) - valid:])
        if cursor < cap:
            assert (ring[cursor:] == -7.0).all()
        for j in range(max(cursor - cap, 0), cursor, 37):
            assert np.array_equal(ring[j % cap], everything[j])
    assert cursor == 883 and cursor // cap == 2
    # a segment longer than the ring keeps its first `capacity` rows, as the kernel clamps its count
    ring2 = np.zeros((cap, 37))
    seg = rng.standard_normal((cap + 11, 37))
    assert ring_append(ring2, 299, seg) == 299 + cap
    assert np.array_equal(ring2[299], seg[0]) and np.array_equal(ring2[298], seg[cap - 1])


def test_abi_exports_and_struct_size(tmp_path):
    from qtos_amd import capi
    lib = capi.load()
    assert "qtos_stitch" in capi.EXPORTS and "qtos_stitch_device" in capi.EXPORTS
    assert hasattr(lib, "qtos_stitch") and hasattr(lib, "qtos_stitch_device")
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qtos_planner.h"\n'
                   'int main(void) { printf("%d %d %d %d %d %d\\n", (int)sizeof(QtosStitch), (int)offsetof(QtosStitch, hz), '
                   '(int)offsetof(QtosStitch, first_row), (int)offsetof(QtosStitch, n_rows), (int)offsetof(QtosStitch, advance_clock), '
                   '(int)offsetof(QtosStitch, capacity)); return 0; }\n')
    exe = tmp_path / "size"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)], text=True).split()]
    S = capi.QtosStitch
    assert got == [C.sizeof(S), S.hz.offset, S.first_row.offset, S.n_rows.offset, S.advance_clock.offset, S.capacity.offset]
    assert C.sizeof(S) == 32
    s = capi.stitch_params(6000, "reference", 12, 500.0, False)
    assert (s.capacity, s.first_row, s.n_rows, s.hz, s.advance_clock) == (6000, 1, 12, 500.0, 0)
    assert capi.stitch_params(10).first_row == 0 and capi.stitch_params(10).advance_clock == 1
    # the argument checks that need no planner
    buf = np.zeros(37)
    cur = np.zeros(1, np.int64)
    ok = capi.stitch_params(1)
    assert lib.qtos_stitch(None, 1, C.byref(ok), capi._dp(buf), None, capi._dp(buf), capi._dp(buf), cur.ctypes.data_as(C.POINTER(C.c_longlong))) == -1
    assert lib.qtos_stitch_device(None, 1, C.byref(ok), None, None, None, None, None, None) == -1


def test_c99_stitch_loop_builds_and_checks_its_arguments(tmp_path):
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
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_stitch"]) == C.sizeof(capi.QtosStitch)
    assert int(kv["stitch_null"]) == -1 and int(kv["stitch_device_null"]) == -1


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """Kernel name -> its metadata block of the code object's notes (as tests/test_kernel_resources.py reads them)."""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s"], env=dict(os.environ, PATH=os.environ.get("PATH", "") + ":/opt/rocm/bin"))
    d = tmp_path_factory.mktemp("co")
    fat, co = str(d / "fat.bin"), str(d / "k.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    out = {}
    for block in text.split("- .agpr_count")[1:]:
        out[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    return out


def field(block, name):
    return int(re.search(r"\.%s:\s+(\d+)" % name, block).group(1))


def one_kernel(notes, kernel):
    names = [n for n in notes if re.search(r"(^|\d)%s(E|$)" % kernel, n)]
    assert len(names) == 1, (kernel, names)
    return notes[names[0]]


STITCH_TILE = 512                  # rows per tile = lanes per workgroup (window_kernels.hpp)


def test_k_stitch_uses_no_scratch_and_one_tile_of_lds(notes):
    block = one_kernel(notes, "k_stitch")
    assert field(block, "private_segment_fixed_size") == 0, "scratch bytes per lane"
    assert field(block, "vgpr_spill_count") == 0
    assert field(block, "max_flat_workgroup_size") == STITCH_TILE
    assert field(block, "vgpr_count") <= 128                     # (512 lanes per workgroup: two waves per SIMD)
    assert field(block, "group_segment_fixed_size") == STITCH_TILE * 37 * 8 <= 160 * 1024


# k_sample's vgpr_count in a build of the parent commit (the commit that added k_handover), read from its code object
# with the lines of the `notes` fixture above
PARENT_K_SAMPLE_VGPRS = 108


def test_k_sample_is_no_larger_than_before_the_row_evaluator_was_shared(notes):
    block = one_kernel(notes, "k_sample")
    assert field(block, "private_segment_fixed_size") == 0
    assert field(block, "vgpr_spill_count") == 0
    assert field(block, "vgpr_count") <= PARENT_K_SAMPLE_VGPRS
