"""The boundary from C: include/qtos_planner.h compiles as C99 under gcc -Wall -Wextra -Werror -pedantic, a C program links against
libqtos_planner.so and calls the host-only entry points (no GPU) -- and the QtosParams image the Python mirror writes is the struct the
C side reads (same size, same offsets: the analysis returns the dimensions capi.analyze returns)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CSRC = os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc")


@pytest.mark.parametrize("name", ["reference_compat", "knots100_trot"])
def test_c99_caller_links_and_sees_the_same_structs(tmp_path, name):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()                                           # (raises with build instructions if the library is missing)
    exe = tmp_path / "abi_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "abi_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cfg = PlannerConfig.reference_compat() if name == "reference_compat" else PlannerConfig.knots100(gait="trot", kappa_sigma=12.5)
    p = capi.params_from_config(cfg)
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(p))
    out = tmp_path / "out.csv"
    r = subprocess.run([str(exe), str(img), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for t in r.stdout.splitlines()[0].split()[1:])
    d, _ = capi.analyze(cfg)
    assert int(kv["rc"]) == 0 and int(kv["sizeof_params"]) == C.sizeof(capi.QtosParams) and int(kv["sizeof_dims"]) == C.sizeof(capi.QtosDims)
    for k in ("n_vars", "n_cons", "n_free", "n_eq", "n_ineq", "n_unknowns", "n_stages", "pivots", "front", "order_rule", "max_active"):
        assert int(kv[k]) == getattr(d, k), (k, kv[k], getattr(d, k))
    assert int(kv["rows"]) == d.n_rows_csv
    assert float(kv["kappa_sigma"]) == cfg.kappa_sigma and C.sizeof(capi.QtosParams) == capi.QtosParams.kappa_sigma.offset + 8
    assert r.stdout.splitlines()[1] == "build_flags=%d" % capi.build_flags()
    assert r.stdout.splitlines()[2] == "write_csv rc=0 bad_path rc=-2 null rc=-1"
    assert open(out).read().splitlines()[:2] == ["3.756,0,0,0.24" + ",0" * 33, "3.757,6.9309e-07" + ",0" * 35]
