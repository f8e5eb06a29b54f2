"""The entry points of the rollout with the force QP from C and in the built library: the header compiles as strict C99 with the
new struct, capi.QtosRolloutQp's image agrees with the C struct by offsetof and begins with QtosRolloutFeet's fields at its
offsets, tests/c/rolloutqp_caller.c compiles under gcc -Wall -Wextra -Werror -pedantic, links, and without a HIP device answers
the argument checks; k_rollout_qp's two instantiations have the LDS DESIGN.md section 6 states ("Rollout with the force QP": 75
doubles per row of the tile and the chain lane's slab of 90), and k_rollout_feet, k_rollout, k_force_qp and k_force_fit the
figures they had.  On the GPU (marked gpu): the caller plans a trot, makes joint rows, rolls out with the clip and with the QP."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LIB = os.path.join(CSRC, "libqtos_planner.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]
PITCH, SLAB = 75, 90


def build_caller(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "rolloutqp_caller"
    cmd = GCC + [os.path.join(ROOT, "tests", "c", "rolloutqp_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
                 "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    img, jimg = tmp_path / "params.bin", tmp_path / "joint.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.knots100(gait="trot"))))
    jimg.write_bytes(bytes(capi.joint_params(hz=200.0, n_rows=800, tau_max=0.0)))
    return exe, img, jimg


def test_exports_constants_and_null_planner(hip_lib):
    from qtos_amd import capi, rollout_qp
    for name in ("qtos_rollout_qp", "qtos_rollout_qp_device"):
        assert hasattr(hip_lib, name) and name in capi.EXPORTS
    assert capi.ROLLOUT_QP_COLS == rollout_qp.QP_COLS == capi.QP_COLS == 8 and capi.ROLLOUT_CAP == rollout_qp.CAP == 512
    assert capi.ROLLOUT_CAP > capi.ROLLOUT_LIMITED and not capi.ROLLOUT_CAP & (2 * capi.ROLLOUT_LIMITED - 1)
    p = capi.rollout_qp_params()
    assert (p.arm, p.damping, p.w_min, p.feet_flags, p.mu_end, p.act_tol, p.max_iter) == (0.2, 1e-6, 0.01, 0, 1e-6, 1e-3, 25) and p.hz == 1000.0
    assert hip_lib.qtos_rollout_qp(None, 1, C.byref(p), *([None] * 16)) == -1
    assert hip_lib.qtos_rollout_qp_device(None, 1, C.byref(p), *([None] * 17)) == -1


def test_c99_caller_compiles_links_and_checks_arguments(tmp_path):
    """The caller prints offsetof of the feet's and the QP's fields and the constants: they are capi.QtosRolloutQp's and capi's."""
    from qtos_amd import capi
    exe, img, jimg = build_caller(tmp_path)
    r = subprocess.run([str(exe), str(img), str(jimg)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    t = lines[0].split()
    got = dict(zip(t[0::2], t[1::2]))
    Q, F = capi.QtosRolloutQp, capi.QtosRolloutFeet
    fields = [name for name, _ in Q._fields_]
    assert fields == [name for name, _ in F._fields_] + ["mu_end", "act_tol", "max_iter"]
    assert all(getattr(Q, f).offset == getattr(F, f).offset for f, _ in F._fields_)
    assert int(got["sizeof"]) == C.sizeof(Q) and int(got["sizeof_feet"]) == C.sizeof(F)
    for f in ("arm", "f_max", "feet_flags"):
        assert got[f] == "%d,%d" % (getattr(Q, f).offset, getattr(F, f).offset)
    for f in ("mu_end", "act_tol", "max_iter"):
        assert int(got[f]) == getattr(Q, f).offset
    assert lines[1] == "constants %d %d %d" % (capi.ROLLOUT_QP_COLS, capi.ROLLOUT_CAP, capi.ROLLOUT_LIMITED)
    assert lines[2] == "rollout_qp_null=-1 rollout_qp_device_null=-1"
    if "no HIP device" not in r.stdout:
        assert lines[3].startswith("bad_args=" + ",".join(["-1"] * 10) + " reason=qtos_rollout_qp: act_tol")


@pytest.fixture(scope="module")
def notes(tmp_path_factory):
    """Kernel name -> its metadata block of the code object's notes (as tests/test_rolloutfeet_caller.py reads them)."""
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


def one(notes, pattern):
    names = [n for n in notes if re.search(pattern, n)]
    assert len(names) == 1, (pattern, sorted(notes))
    return notes[names[0]]


@pytest.mark.parametrize("tile", [256, 64])
def test_rollout_qp_kernel_has_the_stated_lds(notes, tile):
    block = one(notes, r"\d+k_rollout_qpILi%dE" % tile)
    assert PITCH % 2 == 1 and field(block, "group_segment_fixed_size") == tile * PITCH * 8 + SLAB * 8 <= 160 * 1024
    assert field(block, "max_flat_workgroup_size") == tile
    print("k_rollout_qp<%d>" % tile, {f: field(block, f) for f in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")})


def test_the_kernels_it_is_built_from_keep_their_figures(notes):
    """(vgprs, scratch bytes, spilled vector registers, LDS bytes) of the kernels whose device functions k_rollout_qp shares: the
    parent commit's, as scratch/kernel_resources.py prints them for a library built from it."""
    want = {r"\d+k_rollout_feetILi256E": (438, 0, 0, 137216), r"\d+k_rollout_feetILi64E": (438, 0, 0, 34304), r"\d+k_rolloutILi256E": (278, 0, 0, 75776),
            r"\d+k_rolloutILi64E": (276, 0, 0, 18944), r"\d+k_force_qpE": (512, 820, 356, 136192), r"\d+k_force_fitE": (273, 0, 0, 69632)}
    for pattern, figures in want.items():
        block = one(notes, pattern)
        got = tuple(field(block, f) for f in ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size"))
        assert got == figures, (pattern, got, figures)


@pytest.mark.gpu
def test_rollout_qp_from_plain_c(tmp_path):
    exe, img, jimg = build_caller(tmp_path)
    r = subprocess.run(["timeout", "-k", "10", "120", str(exe), str(img), str(jimg)], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout, r.stderr)
    lines = r.stdout.splitlines()
    assert lines[2] == "rollout_qp_null=-1 rollout_qp_device_null=-1"
    assert lines[3].startswith("bad_args=" + ",".join(["-1"] * 10) + " reason=qtos_rollout_qp: act_tol")
    assert lines[4] == "plan rc=0 status=0,0" and lines[5] == "joint rc=0"
    for i, qp in ((6, 0), (7, 1)):
        kv = dict(t.split("=") for t in lines[i].split()[1:])
        assert int(kv["qp"]) == qp and int(kv["rc"]) == 0 and int(kv["mismatches"]) == 0 and int(kv["limited"]) > 0 and float(kv["miss_f"]) > 0
        assert (int(kv["most_steps"]) > 0) == bool(qp) and int(kv["most_steps"]) <= 25 and (qp or int(kv["cap"]) == 0)
