"""The force-QP entry points from C and in the built library: tests/c/forceqp_caller.c compiles under gcc -std=c99 -Wall -Wextra
-Werror -pedantic, links, and without a HIP device answers the argument checks; k_force_qp's and k_force_fit's resources are
what DESIGN.md section 6 states (k_force_fit's are the ones it had before k_force_qp was added).  On the GPU (marked gpu): the
caller plans, makes joint rows, fits with limits and prints the records the Python route answers for the same plans, and
`python -m qtos_amd.main ... --fit-limits MU,FMAX` prints the lines LocalPlanner.solve(fit="limits") prints."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")
LIB = os.path.join(CSRC, "libqtos_planner.so")
LLVM = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")
GCC = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include")]


def build_caller(tmp_path):
    from qtos_amd import capi
    capi.load()
    exe = tmp_path / "forceqp_caller"
    cmd = GCC + [os.path.join(ROOT, "tests", "c", "forceqp_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
                 "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr
    return exe


def test_c99_caller_compiles_links_and_checks_arguments(tmp_path):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    exe = build_caller(tmp_path)
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(PlannerConfig.reference_compat(gait="trot"))))
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split())
    assert int(kv["sizeof_force_qp"]) == C.sizeof(capi.QtosForceQp) == C.sizeof(capi.QtosForceFit) + 40
    assert int(kv["qp_null"]) == -1 and int(kv["qp_device_null"]) == -1
    fields = [name for name, _ in capi.QtosForceQp._fields_]
    assert fields[:len(capi.QtosForceFit._fields_)] == [name for name, _ in capi.QtosForceFit._fields_]
    assert fields[-5:] == ["mu", "f_max", "mu_end", "act_tol", "max_iter"]
    assert all(getattr(capi.QtosForceQp, f).offset == getattr(capi.QtosForceFit, f).offset for f, _ in capi.QtosForceFit._fields_)
    if "no HIP device" not in r.stdout:
        assert "bad_args=-1,-1,-1,-1,-1,-1,-1,-1 reason=qtos_force_qp: arm" in r.stdout, r.stdout


def test_kernel_resources():
    """k_force_qp: 128 lanes, the LDS of DESIGN.md's table; k_force_fit keeps its registers and LDS."""
    import tempfile
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s"], env=dict(os.environ, PATH=os.environ.get("PATH", "") + ":/opt/rocm/bin"))
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               "--input=" + fat, "--output=" + co, "--unbundle"])
        text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    got = {}
    for name in ("k_force_qp", "k_force_fit"):
        blocks = [b for b in text.split("- .agpr_count")[1:] if re.search(r"\.name:\s+\S*\d+%sE" % name, b)]
        assert len(blocks) == 1, name
        got[name] = {f: int(re.search(r"\.%s:\s+(\d+)" % f, blocks[0]).group(1)) for f in
                     ("vgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "group_segment_fixed_size", "max_flat_workgroup_size")}
        print(name, got[name])
    qp, fit = got["k_force_qp"], got["k_force_fit"]
    # the slab of 78 + 12 doubles per lane, the two tiles at their pitches of 33 and 9, the reduction's scratch
    assert qp["group_segment_fixed_size"] == 128 * 8 * (90 + 33 + 9 + 1) and qp["max_flat_workgroup_size"] == 128
    assert fit["group_segment_fixed_size"] == 256 * 33 * 8 + 256 * 8 and fit["vgpr_count"] == 273 and fit["private_segment_fixed_size"] == 0


@pytest.mark.gpu
def test_c_caller_prints_the_summary_of_the_python_route(tmp_path):
    from qtos_amd import capi
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.reference_compat(gait="trot")
    exe = build_caller(tmp_path)
    img, out = tmp_path / "params.bin", tmp_path / "nodes.bin"
    img.write_bytes(bytes(capi.params_from_config(cfg)))
    r = subprocess.run(["timeout", "-k", "10", "300", str(exe), str(img), str(out)], capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "bad_args=-1,-1,-1,-1,-1,-1,-1,-1" in r.stdout and "stamp_mismatches=0 differ=0" in r.stdout and "outside=0" in r.stdout
    assert int(re.search(r"limited_rows=(\d+)", r.stdout).group(1)) > 100
    P = Planner(cfg, max_batch=2)
    try:
        nodes = np.fromfile(str(out), np.float64).reshape(2, P.n)
        _, _, _, summary = P.force_qp(nodes, np.array([0.0, 10.0]), capi.qp_params(cfg, hz=100.0, n_rows=520, mu=0.5, f_max=16.0), rows=False)
    finally:
        P.close()
    got = re.findall(r"window (\d) (\w+) max=\S+ bits=([0-9a-f]+) row=(-?\d+) count=(\d+)", r.stdout)
    assert len(got) == 8
    for b, fam, mx, row, count in got:
        s = summary[int(b)][["res_ang", "res_lin", "change", "limited"].index(fam)]
        bits = int(np.array([s["max"]], np.float64).view(np.int64)[0])
        assert (int(mx, 16), int(row), int(count)) == (bits, int(s["row"]), int(s["count"])), (b, fam, s)


@pytest.mark.gpu
def test_solve_and_command_line_print_the_fit_with_limits(tmp_path, capsys):
    from conftest import load_gv
    from qtos_amd import capi, flags, force_qp as fq
    from qtos_amd.planner import LocalPlanner
    inp = load_gv("gv1")["inputs"]
    args = {"-g": inp["g"], "-s": inp["s"], "-s_ang": [0, 0, 0], "-e1": inp["ee"][0], "-e2": inp["ee"][1],
            "-e3": inp["ee"][2], "-e4": inp["ee"][3], "-t": 3.756, "-resolution": 0.01, "scripts": {}}
    lp = LocalPlanner(max_batch=1)
    try:
        assert lp.solve(args, out_csv=str(tmp_path / "a.csv"), fit="limits", limits=dict(mu=0.3, f_max=12.0)) == 0
        lines = capsys.readouterr().out.splitlines()[-4:]
        summary = lp.last["fit_limits"]
        assert [ln.split()[2] for ln in lines] == list(fq.FAMILIES) and lines == fq.report_lines(summary, 3.756, 1000.0, capi.FIT_TOL)
        _, _, _, want = lp.planner().force_qp(lp.last["nodes"][:1], 3.756, capi.qp_params(lp.cfg, n_rows=5001, mu=0.3, f_max=12.0), rows=False)
        assert summary.tobytes() == want[0].tobytes() and summary["max"][3] > 1.0                 # newtons moved by the cap of 12 N
        assert lp.solve(args, out_csv=str(tmp_path / "b.csv")) == 0 and "fit_limits" not in lp.last
        with pytest.raises(ValueError):
            lp.solve(args, out_csv=None, fit="pyramid")
    finally:
        lp.close()
    assert open(tmp_path / "a.csv", "rb").read() == open(tmp_path / "b.csv", "rb").read()
    cmd = ["timeout", "-k", "10", "300", sys.executable, "-m", "qtos_amd.main"] + flags.cmd_args(args).split() + \
        ["--out", str(tmp_path / "c.csv"), "--fit-limits", "0.3,12"]
    r = subprocess.run(cmd, cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=330)
    assert r.returncode == 0, r.stderr[-3000:]
    out = r.stdout.splitlines()
    assert out[-1] == "status -> 0" and out[-5:-1] == lines
    assert open(tmp_path / "c.csv", "rb").read() == open(tmp_path / "a.csv", "rb").read()
