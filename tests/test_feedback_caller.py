"""The feedback hand-over from plain C (tests/c/feedback_caller.c): it compiles as C99 against the header and links, its argument
checks answer before anything touches a device, and k_start_feedback uses no scratch and no LDS.  The run on a device is
tests/test_gpu_feedback.py::test_feedback_from_plain_c."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LIB = os.path.join(CSRC, "libqtos_planner.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def test_null_arguments_come_back_before_anything_touches_a_device(hip_lib):
    from qtos_amd import capi
    p = capi.feedback_params()
    assert hip_lib.qtos_start_feedback(None, 1, C.byref(p), None, None, None, None, None, None, None, None, None, None, None) == -1
    assert hip_lib.qtos_start_feedback_device(None, 1, C.byref(p), None, None, None, None, None, None, None, None, None, None, None, None) == -1


def test_c99_caller_compiles_links_and_checks_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "feedback_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "feedback_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined", "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.reference_compat())))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_feedback"]) == C.sizeof(capi.QtosFeedback)
    assert int(kv["feedback_null"]) == -1 and int(kv["feedback_device_null"]) == -1


def test_feedback_kernel_uses_no_scratch_and_no_lds(tmp_path):
    """The code object of the built library: ScratchSize 0 (private_segment_fixed_size), no spilled vector registers, no LDS."""
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s"], env=dict(os.environ, PATH=os.environ.get("PATH", "") + ":/opt/rocm/bin"))
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "k.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    blocks = [b for b in text.split("- .agpr_count")[1:] if re.search(r"\.name:\s+\S*\d+k_start_feedbackE", b)]
    assert len(blocks) == 1
    field = lambda name: int(re.search(r"\.%s:\s+(\d+)" % name, blocks[0]).group(1))
    assert field("private_segment_fixed_size") == 0 and field("vgpr_spill_count") == 0 and field("group_segment_fixed_size") == 0
    assert field("max_flat_workgroup_size") == 64
