"""The create-time KKT self-test, the parts that need no GPU: which elimination orders a checked create would try and in what
order (qtos_analyze_candidates), the generator of the self-test's inputs against a restatement of its definition
(include/qtos_planner.h), the entry points from C99 on a machine without a device, and the register budget of the reduction
kernel over the factor panels."""
import ctypes as C
import math
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


def _cfg(name):
    from qtos_amd.config import PlannerConfig
    return {
        "trot 2.5 s, dt 0.05": lambda: PlannerConfig(gait="trot", duration=2.5, dt_base=0.05, dt_dynamic=0.05),
        "walk 2.5 s, dt 0.05": lambda: PlannerConfig(gait="walk", duration=2.5, dt_base=0.05, dt_dynamic=0.05),
        "trot 5 s, dt 0.1": lambda: PlannerConfig(gait="trot", duration=5.0, dt_base=0.1, dt_dynamic=0.1),
        "knots100 trot": lambda: PlannerConfig.knots100(gait="trot"),
        "knots100 walk": lambda: PlannerConfig.knots100(),
        "walk 28 s, dt 0.1": lambda: PlannerConfig(gait="walk", duration=28.0, dt_base=0.1, dt_dynamic=0.1),
    }[name]()


# (rule, front) in trial order: qtos_analyze of the parent commit under QTOS_ORDER = 0 / 1 / 2, sorted by the preference of
# pick_order_rule -- front, stages, continuation records, then 2 before 1 before 0.  The two ties of the table (walk 2.5 s:
# rules 2 and 1 on 96 slots; knots100 trot: rules 2 and 0 on 96 slots) have equal stage counts (63 / 113) and no continuation
# records on either side, so "2 before 1 before 0" decides them: the order below is the table's.
CANDIDATES = {
    "trot 2.5 s, dt 0.05": ([(2, 96), (1, 112)], [(0, 80), (2, 96), (1, 112)]),
    "walk 2.5 s, dt 0.05": ([(2, 96), (1, 96)], [(0, 80), (2, 96), (1, 96)]),
    "trot 5 s, dt 0.1": ([(2, 96), (1, 112)], [(0, 80), (2, 96), (1, 112)]),
    "knots100 trot": ([(2, 96), (1, 112)], [(2, 96), (0, 96), (1, 112)]),
    "knots100 walk": ([(1, 96), (2, 112)], [(1, 96), (2, 112), (0, 112)]),
    "walk 28 s, dt 0.1": ([(1, 160), (2, 192)], [(1, 160), (2, 192), (0, 192)]),
}


@pytest.fixture()
def no_order_env(monkeypatch):
    monkeypatch.delenv("QTOS_ORDER", raising=False)


@pytest.mark.parametrize("name", sorted(CANDIDATES))
def test_candidates_are_the_recorded_table_and_start_from_the_plain_choice(name, no_order_env, monkeypatch):
    from qtos_amd import capi
    cfg = _cfg(name)
    auto, every = CANDIDATES[name]
    got0, got7 = capi.analyze_candidates(cfg, 0), capi.analyze_candidates(cfg, 7)
    assert [(r, f) for r, f, _ in got0] == auto, got0
    assert [(r, f) for r, f, _ in got7] == every, got7
    d, _ = capi.analyze(cfg)
    assert (d.order_rule, d.front, d.n_stages) == got0[0]      # the checked create starts from the planner the plain create builds
    # every candidate is the analysis QTOS_ORDER gives for its rule
    for rule, front, stages in got7:
        monkeypatch.setenv("QTOS_ORDER", str(rule))
        dr, _ = capi.analyze(cfg)
        assert (dr.order_rule, dr.front, dr.n_stages) == (rule, front, stages)
        monkeypatch.delenv("QTOS_ORDER")
    # a mask selects among them and keeps the order
    assert capi.analyze_candidates(cfg, 5) == [c for c in got7 if c[0] in (0, 2)]
    monkeypatch.setenv("QTOS_ORDER", "0")
    for mask in (0, 2, 7):
        only = capi.analyze_candidates(cfg, mask)
        assert [c[0] for c in only] == [0] and only[0] in got7, (mask, only)


def test_full_base_systems_have_rule_0_alone(no_order_env):
    """Rules 1 and 2 move the coefficients of a reduced base: without it the automatic choice is rule 0, and so is the
    candidate list whatever the mask."""
    import dataclasses
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    cfg = dataclasses.replace(PlannerConfig.reference_compat(), reduce_base=False, reduce_swing=False)
    d, _ = capi.analyze(cfg)
    assert d.order_rule == 0
    for mask in (0, 6, 7):
        assert capi.analyze_candidates(cfg, mask) == [(0, d.front, d.n_stages)]


# ---- the generator, restated from the header's comment ------------------------------------------------------------------------
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _mix(z):
    z = np.asarray(z, np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _bits(seed, problem, array, idx):
    key = _mix(_mix(_mix(np.uint64(seed)) ^ np.uint64(problem)) ^ np.uint64(array))
    return _mix(key ^ np.asarray(idx, np.uint64))


def _uniform(seed, problem, array, idx):
    return ((_bits(seed, problem, array, idx) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def _normal(seed, problem, array, count):
    i = np.arange(count, dtype=np.uint64)
    u1, u2 = _uniform(seed, problem, array, 2 * i), _uniform(seed, problem, array, 2 * i + 1)
    # (libm through the math module: glibc's log / cos on both sides; numpy's vector versions need not round alike)
    return np.array([math.sqrt(-2.0 * math.log(a)) * math.cos(6.283185307179586 * b) for a, b in zip(u1, u2)])


def _restated(seed, problem, n, m):
    dx0 = 0.01 * _normal(seed, problem, 0, n)
    sig = np.array([math.pow(10.0, -3.0 + 6.0 * u) for u in _uniform(seed, problem, 1, np.arange(m))])
    w = _normal(seed, problem, 2, m) * np.sqrt(sig)
    return dx0, sig, w


def _ulps(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def test_selftest_inputs_are_the_generator_of_the_header(no_order_env):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig.knots100(gait="trot")
    d, _ = capi.analyze(cfg)
    for seed, problem, array in ((0, 0, 0), (0, 1, 1), (2026, 1, 2), (2 ** 63 + 5, 0, 1)):
        idx = np.array([0, 1, 2, 3, 1000, 2 ** 32 + 7], np.uint64)
        assert [capi.selftest_bits(seed, problem, array, int(i)) for i in idx] == [int(v) for v in _bits(seed, problem, array, idx)]
    for seed, problem in ((0, 0), (0, 1), (7, 1)):
        dx0, sig, w = capi.selftest_inputs(cfg, seed, problem)
        assert dx0.shape == (d.n_vars,) and sig.shape == w.shape == (d.n_cons,)
        r_dx0, r_sig, r_w = _restated(seed, problem, d.n_vars, d.n_cons)
        worst = [float(_ulps(a, b).max()) for a, b in ((dx0, r_dx0), (sig, r_sig), (w, r_w))]
        print("seed %d problem %d: largest distance to the restatement in ulp: dx0 %.1f, sig %.1f, w %.1f" % ((seed, problem) + tuple(worst)))
        assert max(worst) <= 4.0, worst
        assert sig.min() >= 1e-3 and sig.max() <= 1e3
        # N(0, 1): the mean within 5 / sqrt(n), the variance within 5 sqrt(2 / n)
        for z in (w / np.sqrt(sig), dx0 / 0.01):
            n = z.size
            assert abs(z.mean()) < 5.0 / math.sqrt(n) and abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / n), (n, z.mean(), z.var())
        # six decades, evenly: log10(sig) is U(-3, 3) -- mean 0 within 5 sqrt(3 / n), variance 3 within 5 * 3 sqrt(0.8 / n)
        lg = np.log10(sig)
        assert abs(lg.mean()) < 5.0 * math.sqrt(3.0 / lg.size) and abs(lg.var() - 3.0) < 15.0 * math.sqrt(0.8 / lg.size)
    a, b, c = capi.selftest_inputs(cfg, 11, 0), capi.selftest_inputs(cfg, 11, 0), capi.selftest_inputs(cfg, 12, 0)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and not np.array_equal(x, z)
    assert not np.array_equal(capi.selftest_inputs(cfg, 11, 1)[1], a[1])      # (the two problems differ)


def test_selftest_problem_is_the_rest_start_in_nominal_stance():
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig(gait="walk", duration=8.0)
    start, goal = capi.selftest_problem(cfg)
    feet = np.array(cfg.nominal_stance)
    assert np.array_equal(start[:6], [0, 0, -feet[0, 2], 0, 0, 0]) and np.array_equal(start[18:], np.zeros(6))
    assert np.array_equal(start[6:18].reshape(4, 3), feet * [1, 1, 0])
    assert abs(goal[0] - 0.09 * 8.0) < 1e-12 and goal[1] == 0 and goal[2] == start[2]


# ---- from C, without a device ----------------------------------------------------------------------------------------------
def test_c99_caller_sees_the_struct_and_the_error_codes(tmp_path, no_order_env):
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    capi.load()
    exe = tmp_path / "selftest_caller"
    cmd = ["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "c", "selftest_caller.c"), "-o", str(exe), "-L", CSRC, "-lqtos_planner",
           "-Wl,-rpath," + CSRC, "-Wl,--allow-shlib-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    cfg = PlannerConfig.knots100(gait="trot")
    img = tmp_path / "params.bin"
    img.write_bytes(bytes(capi.params_from_config(cfg)))
    # (no device for the child, wherever the test runs: the create must answer -2 before any self-test)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([str(exe), str(img)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout, r.stderr)
    kv = dict(t.split("=") for ln in r.stdout.splitlines() for t in ln.split())
    assert int(kv["sizeof_selftest"]) == C.sizeof(capi.QtosSelftest) == 72
    # (the layouts the self-test's result does not travel in stay what they were; QtosParams: 1440 + the double kappa_sigma,
    #  appended behind everything that was there)
    assert capi.QtosParams.kappa_sigma.offset == 1440
    assert int(kv["sizeof_params"]) == C.sizeof(capi.QtosParams) == 1448 and int(kv["sizeof_dims"]) == C.sizeof(capi.QtosDims) == 128
    assert int(kv["selftest_null"]) == -1 and int(kv["selftest_null_out"]) == -1
    assert int(kv["checked"]) == -2 and int(kv["out_null"]) == 1 and int(kv["n_tried"]) == 0
    assert int(kv["checked_null_params"]) == -1
    first = capi.analyze_candidates(cfg, 0)
    assert (int(kv["n_candidates"]), int(kv["first_rule"]), int(kv["first_front"]), int(kv["first_stages"])) == (len(first),) + first[0]
    assert int(kv["bits"]) == int(_bits(1, 0, 2, np.uint64(3)))
    assert "no HIP device" in r.stderr


def test_checked_create_without_a_device_fails_like_the_plain_create(no_order_env):
    """-2 from either: the same RuntimeError text class, not SelftestError.  In a child process that sees no device, wherever
    the suite runs."""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from qtos_amd import capi\n"
            "from qtos_amd.config import PlannerConfig\n"
            "cfg = PlannerConfig.knots100(gait='trot')\n"
            "for kw in (dict(), dict(checked=True), dict(checked=True, rules_mask=7)):\n"
            "    try:\n"
            "        capi.Planner(cfg, max_batch=2, **kw)\n"
            "        print('created')\n"
            "    except capi.SelftestError as e:\n"
            "        print('SelftestError', e)\n"
            "    except RuntimeError as e:\n"
            "        print('RuntimeError', e)\n" % ROOT)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 3 and all(ln.startswith("RuntimeError ") and "(-2)" in ln for ln in lines), lines
    assert lines[0].split("failed", 1)[1] == lines[1].split("failed", 1)[1] == lines[2].split("failed", 1)[1]
    assert "qtos_planner_create failed" in lines[0] and "qtos_planner_create_checked failed" in lines[1]


def test_selftest_error_carries_the_attempts():
    from qtos_amd import capi
    t = capi.QtosSelftest(order_rule=0, front=80, n_stages=75, n_problems=2, worst_stage=2, passed=0, residual=6.5e-3, max_factor=5.17e9)
    e = capi.SelftestError([t, capi.QtosSelftest(order_rule=1)])
    assert isinstance(e, RuntimeError) and e.attempts[0].worst_stage == 2
    assert "rule 0, residual 6.5e-03, max |V| 5.17e+09, rejected (stage 2)" in str(e) and "rule 1, not built" in str(e)


def test_report_header_gains_the_selftest_line_only_for_a_checked_planner():
    from qtos_amd import capi, report
    d = capi.QtosDims()
    rep = capi.QtosReport()
    rows = np.zeros((1, capi.HIST_COLS))
    rows[0, 2] = 0.1
    plain = report.format_report(d, (0, 0), rep, rows, 24)
    assert plain == report.format_report(d, (0, 0), rep, rows, 24, selftests=[])
    t = capi.QtosSelftest(order_rule=2, front=96, passed=1, residual=4.0e-9, max_factor=1.0e8)
    checked = report.format_report(d, (0, 0), rep, rows, 24, selftests=[capi.QtosSelftest(order_rule=0, front=80), t])
    a, b = plain.splitlines(), checked.splitlines()
    assert b[1] == "KKT self-test: rule 2, residual 4.0e-09, max |V| 1.00e+08, passed"
    assert b[:1] + b[2:] == a


# ---- the reduction kernel's code object -----------------------------------------------------------------------------------
def test_panel_reduction_kernel_uses_no_scratch(tmp_path):
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", CSRC, "-s"], env=dict(os.environ, PATH=os.environ.get("PATH", "") + ":/opt/rocm/bin"))
    fat, co = str(tmp_path / "fat.bin"), str(tmp_path / "k.co")
    subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB])
    subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           "--input=" + fat, "--output=" + co, "--unbundle"])
    text = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    blocks = {}
    for block in text.split("- .agpr_count")[1:]:
        blocks[re.search(r"\.name:\s+(\S+)", block).group(1)] = block
    names = [n for n in blocks if re.search(r"(^|\d)k_panel_absmax(E|$)", n)]
    assert len(names) == 1, sorted(blocks)

    def field(name):
        return int(re.search(r"\.%s:\s+(\d+)" % name, blocks[names[0]]).group(1))
    assert field("private_segment_fixed_size") == 0
    assert field("vgpr_spill_count") == 0 and field("sgpr_spill_count") == 0
    # (the evaluation kernels the existing budget test reads are still found exactly once each)
    for kernel in ("k_step", "k_start", "k_shift_warm"):
        assert len([n for n in blocks if re.search(r"(^|\d)%s(E|$)" % kernel, n)]) == 1, kernel
