"""Every factor + solve kernel the product library can select (QTOS_KKT, include/qtos_planner.h: qtos_kkt_kernel) on the
driver's box: k_kkt2 (forced: 2), k_kkt3 MODE 1 (forced: 4; the default up to 112 slots) and k_kkt5 (6: two 16-pivot stages
per set of barriers, pair-mode analysis).  The kernels that were built, measured and lost (k_kkt3 MODE 0, k_kkt4) left csrc/ in
round 6 (scratch/experiments/); the environment is read once per planner (csrc/env.hpp) and read back through qtos_env."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _planner(cfg, B, kkt):
    from qtos_amd.capi import Planner, analyze_kernel
    old = os.environ.get("QTOS_KKT")
    if kkt is None:
        os.environ.pop("QTOS_KKT", None)
    else:
        os.environ["QTOS_KKT"] = kkt
    try:
        P = Planner(cfg, max_batch=B)
        assert P.kkt_kernel() == analyze_kernel(cfg)     # (the host-only entry point makes the same choice)
        return P
    finally:
        if old is None:
            os.environ.pop("QTOS_KKT", None)
        else:
            os.environ["QTOS_KKT"] = old


def _workload(name, B):
    from qtos_amd import workloads
    from qtos_amd.config import PlannerConfig
    if name == "walk":
        return PlannerConfig.knots100(), None, workloads.flat_goals(B, seed=0) + (None,)
    if name == "trot":
        return PlannerConfig.knots100(gait="trot"), None, workloads.flat_goals(B, seed=0) + (None,)
    if name == "reference_compat":
        # (the trot of the reference's own transcription: its walk needs continuation records under the order with the early
        #  coefficients -- rule 2, round 6 -- and runs k_kkt2 whatever is asked for)
        return PlannerConfig.reference_compat(gait="trot"), None, workloads.flat_goals(B, seed=1) + (None,)
    ter = workloads.mixed_terrains()
    start, goal, mid = workloads.mixed_goals(B, seed=9, terrains=ter)
    return PlannerConfig.knots100(), ter, (start, goal, mid)


EXPECT = {   # kernel each choice resolves to on the front of the workload (reduced swings + short stages + round 6's order with the late
             # force nodes where it is the smaller one: walk 96 slots (112 by the order of rounds 1 - 5), trot 96; pair-mode analysis of
             # k_kkt5: 112 / 112)
    ("2", "walk"): "k_kkt2<96>", ("4", "walk"): "k_kkt3<96, 1>", ("6", "walk"): "k_kkt5<112>", (None, "walk"): "k_kkt3<96, 1>",
    ("2", "trot"): "k_kkt2<96>", ("4", "trot"): "k_kkt3<96, 1>", ("6", "trot"): "k_kkt5<112>", (None, "trot"): "k_kkt3<96, 1>",
    ("2", "mixed"): "k_kkt2<96>", ("4", "mixed"): "k_kkt3<96, 1>", ("6", "mixed"): "k_kkt5<112>", (None, "mixed"): "k_kkt3<96, 1>",
}


@pytest.mark.parametrize("workload", ["walk", "trot", "mixed"])
@pytest.mark.parametrize("kkt", ["2", "4", "6"])
def test_every_selectable_kernel_matches_the_oracle(kkt, workload):
    """B = 32 problems through the forced kernel: all converge, the kernel that ran is the one asked for, and 8 of them equal the
    oracle's plans (same iteration counts, nodes to 1e-6 on every workload: the trot's 5e-6 of rounds 3 - 5 was the elimination order of those
    rounds)."""
    from test_gpu_parity import _batch_vs_oracle
    B = 32
    cfg, ter, (start, goal, mid) = _workload(workload, B)
    P = _planner(cfg, B, kkt)
    assert P.kkt_kernel() == EXPECT[(kkt, workload)], P.kkt_kernel()
    if ter is not None:
        P.set_heightfields(ter[0], ter[1])
    nodes, status, iters, viol = P.plan(start, goal, map_id=mid)
    P.close()
    assert (status == 0).all() and viol.max() <= cfg.tol
    tol = 1e-6
    same, worst = _batch_vs_oracle(cfg, start, goal, range(0, B, 4), maps=None if ter is None else ter[0], cell=None if ter is None else ter[1],
                                   map_id=mid, status=status, iters=iters, nodes=nodes, tol=tol)
    assert same == 8, (same, worst)


@pytest.mark.parametrize("workload", ["trot", "reference_compat", "mixed"])
def test_k_kkt3_mode_1_gives_the_bits_of_k_kkt2(workload):
    """k_kkt3 MODE 1 is k_kkt2's arithmetic on another schedule (the assembly on the waves that idle in phase AB): nodes,
    status, iterations and violations are equal bit for bit -- the claim the default for fronts of at most 112 slots rests on."""
    B = 64
    cfg, ter, (start, goal, mid) = _workload(workload, B)
    res = {}
    for kkt in ("2", "4"):
        P = _planner(cfg, B, kkt)
        assert P.kkt_kernel().startswith("k_kkt2" if kkt == "2" else "k_kkt3")
        if ter is not None:
            P.set_heightfields(ter[0], ter[1])
        res[kkt] = P.plan(start, goal, map_id=mid)
        P.close()
    for a, b in zip(res["2"], res["4"]):
        assert np.array_equal(a, b)


def test_default_selection_and_fallback():
    """Unset: k_kkt3 MODE 1 up to 112 slots (the benchmark's transcriptions), k_kkt2 above (`-duration 12` and longer).  A choice that is not applicable (k_kkt5 on a horizon whose pair-mode
    front has no instantiation, an experiment that left the library) falls back to the default instead of failing."""
    from qtos_amd.config import PlannerConfig
    for workload in ("walk", "trot"):
        cfg, _, _ = _workload(workload, 4)
        P = _planner(cfg, 4, None)
        assert P.kkt_kernel() == EXPECT[(None, workload)]
        P.close()
    P = _planner(PlannerConfig.reference_compat(duration=20.0), 2, "6")
    assert P.kkt_kernel().startswith("k_kkt2")       # (`-duration 20`: a front of 160 slots and more, no k_kkt5 for it)
    P.close()
    P = _planner(PlannerConfig.knots100(), 2, "5")
    assert P.kkt_kernel() == EXPECT[(None, "walk")]
    P.close()


def test_environment_is_read_once_at_creation_and_read_back():
    """Round 6: every QTOS_* switch is parsed in one place when the planner is created (csrc/env.hpp) and the handle says what it
    runs with (qtos_env); a change of the environment behind an existing handle does not reach it."""
    import os
    from qtos_amd.config import PlannerConfig
    P0 = _planner(PlannerConfig.knots100(), 2, None)
    e0 = P0.env()
    assert e0["QTOS_KKT"] == "0" and e0["QTOS_LANES"] == "1" and e0["QTOS_SHORT_STAGES"] == "unset" and e0["QTOS_SPEC_PATTERN"] == "1"
    assert e0["QTOS_SWEEP_DS"] == "1" and e0["QTOS_SPEC_JAC"] == "1" and e0["QTOS_ORDER"] == "unset"
    old = {k: os.environ.get(k) for k in ("QTOS_KKT", "QTOS_LANES", "QTOS_SPEC_PATTERN", "QTOS_SHORT_STAGES", "QTOS_ORDER")}
    os.environ.update(QTOS_KKT="2", QTOS_LANES="3", QTOS_SPEC_PATTERN="0", QTOS_SHORT_STAGES="0", QTOS_ORDER="0")
    try:
        assert P0.env() == e0 and P0.kkt_kernel() == EXPECT[(None, "walk")]     # the old handle keeps what it was created with
        from qtos_amd.capi import Planner, analyze_kernel
        P1 = Planner(PlannerConfig.knots100(), max_batch=2)
        assert P1.kkt_kernel() == analyze_kernel(PlannerConfig.knots100())
        e1 = P1.env()
        assert (e1["QTOS_KKT"], e1["QTOS_LANES"], e1["QTOS_SPEC_PATTERN"], e1["QTOS_SHORT_STAGES"], e1["QTOS_ORDER"]) == ("2", "3", "0", "0", "0")
        assert P1.kkt_kernel().startswith("k_kkt2<128") and P1.dims.front == 128     # (the order of rounds 1 - 5 without short stages: the walk's 128 slots; k_kkt2 forced)
        P1.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    P0.close()


@pytest.mark.parametrize("kkt", ["2", "6"])
def test_factor_panels_of_either_kernel_match_the_block_elimination(kkt, oracle, gv1, cfg):
    """test_gpu_parity.check_factor_panels (w and V of every ninth stage against a numpy block elimination in the planner's own
    elimination order, full system of the reference's NLP) through k_kkt2 and through k_kkt5: the pair kernel leaves the same
    per-stage panels for k_chord and the sweeps."""
    import dataclasses
    from test_gpu_parity import check_factor_panels
    P = _planner(dataclasses.replace(cfg, reduce_base=False, reduce_swing=False), 8, kkt)
    assert P.kkt_kernel().startswith("k_kkt5" if kkt == "6" else "k_kkt2")
    check_factor_panels(P, oracle, gv1, cfg)
    P.close()


@pytest.mark.parametrize("gait,duration,dt", [("trot", 2.5, 0.05), ("trot", 5.0, 0.1), ("trot", 2.5, 0.1), ("trot", 5.0, 0.05), ("trot", 8.0, 0.1),
                                               ("walk", 2.5, 0.05), ("walk", 5.0, 0.1), ("walk", 5.0, 0.05), ("walk", 8.0, 0.1)])
def test_one_kkt_solve_is_accurate_on_every_transcription(gait, duration, dt):
    """The fuzz of round 6 as a test (profiles/r06_experiments/order_fuzz.log, order_rule2.log): one KKT solve with barrier weights
    over six decades, in the elimination order the planner picks for the transcription, has a residual max |b - K x| / max |b|
    below 1e-6 (measured: 4e-11 .. 5e-8; the order of rounds 1 - 5 gave 6.5e-3 on the 2.5 s trot at 0.05 s knots and 1.2e-3 on
    reference_compat's trot), one step of refinement takes it to 1e-11, and no entry of the factor panels exceeds 1 / eps_dual.
    The first three cases are the ones that failed; the order of rounds 1 - 5 (QTOS_ORDER=0) still fails the first there."""
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    cfg = PlannerConfig(gait=gait, duration=duration, dt_base=dt, dt_dynamic=dt)

    def solve(order):
        old = os.environ.get("QTOS_ORDER")
        if order is not None:
            os.environ["QTOS_ORDER"] = order
        try:
            P = Planner(cfg, max_batch=2)
        finally:
            if old is None:
                os.environ.pop("QTOS_ORDER", None)
            else:
                os.environ["QTOS_ORDER"] = old
        s, gl = workloads.flat_goals(2, seed=11)
        gl[:, 0] = s[:, 0] + (gl[:, 0] - s[:, 0]) * (cfg.duration / 5.0)
        x0 = P.initial_guess(s, gl)
        rng = np.random.default_rng(0)
        x = x0 + 0.01 * rng.standard_normal(x0.shape)
        sig = 10.0 ** rng.uniform(-3, 3, (2, P.m))
        w = rng.standard_normal((2, P.m)) * np.sqrt(sig)
        P.debug_newton(s, gl, x, sig, w)
        _, res = P.debug_residual(2, refine=False)
        _, res2 = P.debug_residual(2, refine=True)
        pan, _ = P.factor(0)
        rule = P.dims.order_rule
        P.close()
        return rule, float(res.max()), float(res2.max()), float(np.abs(pan[:, 1:, :]).max())

    rule, res, res2, vmax = solve(None)
    assert rule in (1, 2), rule                     # (a reduced base: rule 0 is not in the automatic choice)
    assert res < 1e-6 and res2 < 1e-11 and vmax <= 1.05 / cfg.eps_dual, (rule, res, res2, vmax)
    if (gait, duration, dt) == ("trot", 2.5, 0.05):
        rule0, res0, _, vmax0 = solve("0")
        assert rule0 == 0 and res0 > 1e-4 and vmax0 > 10.0 / cfg.eps_dual, (res0, vmax0)   # the finding itself stays on record
