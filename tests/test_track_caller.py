"""The track entry points from C and in the built library (no GPU): tests/c/track_caller.c compiles as C99 under gcc -Wall -Wextra
-Werror -pedantic against include/qtos_planner.h, links, and without a HIP device answers the argument checks; the struct the
Python mirror writes is the struct the C side reads; k_track's two instantiations run without scratch, with the LDS DESIGN.md
section 6 states."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LIB = os.path.join(CSRC, "libqtos_planner.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def test_exports_and_struct(hip_lib):
    from qtos_amd import capi, joints, tracking
    for name in ("qtos_track", "qtos_track_device"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    p = capi.track_params()
    assert p.capacity == 0 and p.hz == 1000.0 and p.ee_shift == 0.015 and p.delay == 500 and p.flags == 0
    assert [list(r) for r in p.hip] == joints.SOLO12.hip.tolist() and list(p.lateral) == joints.SOLO12.lateral.tolist()
    assert p.l_upper == p.l_lower == 0.16
    assert capi.track_params(quaternion=True).flags == capi.TRACK_QUAT == tracking.FLAG_QUAT
    assert capi.track_params(rule="clean").flags == capi.TRACK_CLEAN_DELAY == tracking.FLAG_CLEAN_DELAY
    assert capi.TRACK_COLS == tracking.TRACK_COLS == 26
    with pytest.raises(ValueError):
        capi.track_params(rule="other")
    # argument errors come back as -1 before anything touches a device
    assert hip_lib.qtos_track(None, 1, C.byref(p), None, None, None, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.qtos_track_device(None, 1, C.byref(p), None, None, None, None, None, None, None, None, None, None, None, None) == -1


def test_sizeof_is_the_c_sizeof(tmp_path):
    from qtos_amd import capi
    src, exe = tmp_path / "size.c", tmp_path / "size"
    src.write_text('#include <stdio.h>\n#include "qtos_planner.h"\nint main(void) { printf("%d\\n", (int)sizeof(QtosTrack)); return 0; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(subprocess.check_output([str(exe)], text=True)) == C.sizeof(capi.QtosTrack)


def test_c99_caller_compiles_links_and_checks_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "track_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "track_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_track"]) == C.sizeof(capi.QtosTrack)
    assert int(kv["track_null"]) == -1 and int(kv["track_device_null"]) == -1


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """Kernel name -> its metadata block of the code object's notes (as tests/test_joint_caller.py reads them)."""
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


@pytest.mark.parametrize("tile,lds", [(512, 512 * 26 * 8), (64, 64 * 26 * 8)])
def test_track_kernel_uses_no_scratch(notes, tile, lds):
    names = [n for n in notes if re.search(r"\d+k_trackILi%dE" % tile, n)]
    assert len(names) == 1, sorted(notes)
    block = notes[names[0]]
    assert field(block, "private_segment_fixed_size") == 0 and field(block, "vgpr_spill_count") == 0
    assert field(block, "group_segment_fixed_size") == lds
