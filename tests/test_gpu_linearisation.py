"""The linearisation (eval_all<true> in csrc/kernels.hpp: what k_start, k_step and k_debug_eval turn a node vector into) against
the oracle on every transcription of linearisation_cases.py, directly: no Newton iteration in between that converges anyway.

  (a) constraint values and the node-space Jacobian of the full system on flat ground, every case, non-zero patterns included
  (b) the same on a stack of three maps with a map index per problem, bilinear and nearest-cell, walk and trot
  (c) the values of the reduced system (reduce_base, reduce_swing: what every benchmark workload runs), every case
  (d) the reduced system's Jacobian through its Newton step at a generic point: the steps of the three reduced systems against
      the full system's, gated by the eps_dual x multiplier gap computed with numpy in the same test

Gates: 1e-10 on values and entries, 1e-9 on entries in bilinear mode -- the figures at the top of test_gpu_parity.py; (d): 8 x
the computed gap.  The oracle's Jacobian is held to difference quotients in test_linearisation_cpu.py.  Every test prints its
figures (linearisation_cases.record) before it asserts."""
import dataclasses

import numpy as np
import pytest

import linearisation_cases as lc
# the dense Newton step (LAPACK, refined in extended precision): it lives with the rest of the interior-point restatement
from oracle.ipm import direction as _dense_step

pytestmark = pytest.mark.gpu


def _batch(name):
    """B = 3 evaluation points; 2 above 3000 variables (the dense host Jacobians stay under 250 MB)."""
    return 2 if lc.case(name)[1].n > 3000 else 3


@pytest.mark.parametrize("name", lc.NAMES)
def test_values_and_jacobian_match_oracle_on_flat_ground(name):
    from qtos_amd.capi import Planner
    cfg, O, L = lc.case(name)
    B = _batch(name)
    x, start, goal = lc.points(name, B, 21)
    P = Planner(lc.full(cfg), max_batch=B)
    try:
        g, J = P.debug_eval(start, goal, x)
        rk, vf, _ = P.structure()
    finally:
        P.close()
    fx = lc.fixed(name)
    assert np.array_equal(vf == 0, fx)
    worst = dict(values=0.0, entries=0.0, pattern_equal=True)
    for b in range(B):
        d = lc.compare(g[b], J[b], O.constraints(x[b]), lc.mask_jacobian(O.jacobian(x[b]), fx, rk), pattern=True)
        worst = dict(values=max(worst["values"], d["values"]), entries=max(worst["entries"], d["entries"]),
                     pattern_equal=worst["pattern_equal"] and d["pattern_equal"])
    lc.record("gpu_flat", name, dict(problems=B, gate_values=lc.GATE_VALUE, gate_entries=lc.GATE_ENTRY,
                                     largest_entry=float(np.abs(J).max()), coef_in_lds=lc.COEF_IN_LDS[name], **worst))
    assert worst["values"] < lc.GATE_VALUE
    assert worst["entries"] < lc.GATE_ENTRY
    assert worst["pattern_equal"]


@pytest.mark.parametrize("mode", [0, 1], ids=["bilinear", "nearest"])
@pytest.mark.parametrize("name", ["walk", "trot"])
def test_values_and_jacobian_match_oracle_on_a_stack_of_maps(name, mode):
    """workloads.mixed_terrains(): three maps on one grid, problem b on map (2, 0, 1)[b], an oracle per map.  No pattern check
    in bilinear mode (a slope may be exactly zero).  A kernel that ignored the map index would pass on a coincidence if the
    maps gave the same rows: the rows of every problem differ from those the oracle of another map gives at the same point."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    cfg = dataclasses.replace(lc.full(lc.case(name)[0]), terrain_mode=mode)
    maps, cell = workloads.mixed_terrains()
    map_id = np.array([2, 0, 1], np.int32)
    Os = [Oracle(oracle_dict(cfg), height=maps[k], hcell=cell) for k in range(3)]
    x, start, goal = lc.points(name, 3, 23, spread=lc.FOOTHOLD_SPREAD)
    P = Planner(cfg, max_batch=3)
    try:
        P.set_heightfields(maps, cell)
        g, J = P.debug_eval(start, goal, x, map_id=map_id)
        rk, vf, _ = P.structure()
    finally:
        P.close()
    fx = lc.fixed(name)
    assert np.array_equal(vf == 0, fx)
    gate_entries = lc.GATE_ENTRY_BILINEAR if mode == 0 else lc.GATE_ENTRY
    worst, other_map = dict(values=0.0, entries=0.0, pattern_equal=True), np.inf
    for b in range(3):
        O = Os[map_id[b]]
        d = lc.compare(g[b], J[b], O.constraints(x[b]), lc.mask_jacobian(O.jacobian(x[b]), fx, rk), pattern=True)
        worst = dict(values=max(worst["values"], d["values"]), entries=max(worst["entries"], d["entries"]),
                     pattern_equal=worst["pattern_equal"] and d["pattern_equal"])
        other_map = min(other_map, min(float(np.abs(g[b] - Os[k].constraints(x[b])).max()) for k in range(3) if k != map_id[b]))
    lc.record("gpu_maps_" + ("bilinear" if mode == 0 else "nearest"), name,
              dict(problems=3, gate_values=lc.GATE_VALUE, gate_entries=gate_entries, largest_entry=float(np.abs(J).max()),
                   distance_from_another_maps_rows=other_map, **worst))
    assert worst["values"] < lc.GATE_VALUE
    assert worst["entries"] < gate_entries
    if mode == 1:
        assert worst["pattern_equal"]
    assert other_map > lc.GATE_VALUE


@pytest.mark.parametrize("name", lc.NAMES)
def test_values_of_the_reduced_system_match_oracle(name):
    """reduce_base and reduce_swing on (the default): other dimensions of the KKT system and other term tables, the same
    arithmetic of the values, at the same points as on flat ground above."""
    from qtos_amd import capi
    cfg, O, L = lc.case(name)
    assert cfg.reduce_base and cfg.reduce_swing
    B = _batch(name)
    x, start, goal = lc.points(name, B, 21)
    P = capi.Planner(cfg, max_batch=B)
    try:
        n_unknowns = P.dims.n_unknowns
        g, _ = P.debug_eval(start, goal, x, jac=False)
    finally:
        P.close()
    assert n_unknowns < capi.analyze(lc.full(cfg))[0].n_unknowns
    err = max(float(np.abs(g[b] - O.constraints(x[b])).max()) for b in range(B))
    lc.record("gpu_reduced_values", name, dict(problems=B, gate_values=lc.GATE_VALUE, values=err))
    assert err < lc.GATE_VALUE


REDUCED = ((True, False), (False, True), (True, True))       # (reduce_base, reduce_swing)


@pytest.mark.parametrize("terrain", ["flat", "maps"])
@pytest.mark.parametrize("name", ["walk", "trot"])
def test_reduced_systems_give_the_newton_step_of_the_full_system_at_a_generic_point(name, terrain):
    """test_reduced_base_system_gives_the_newton_step_of_the_full_system runs at towr's straight-line guess on flat ground:
    every Euler angle and rate zero, equal forces, the rotation-dependent blocks of the Jacobian trivial.  Here: the noisy
    points of linearisation_cases.points, put into the reduced space on the host (oracle.projection.project_nodes, then the
    swing rule), on flat ground and on the three nearest-cell maps with a map index per problem.  The reduced systems' steps
    equal the full system's up to eps_dual x the multipliers of the eliminated rows; that gap is computed here -- the dense KKT
    system of the oracle's Jacobian solved with eps_dual on every equality row, and with 1e-13 on the rows a reduced planner no
    longer marks as equality rows -- and the gate is 8 x the gap, never below the full GPU step's own distance from the dense
    solution.  (At the straight-line guess the existing test holds 1e-7.)"""
    from oracle.oracle import Oracle, oracle_dict
    from oracle.projection import project_nodes
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    cfg, O, L = lc.case(name)
    B = 2
    rng = np.random.default_rng(29)
    fx = lc.fixed(name)
    if terrain == "maps":
        maps, cell = workloads.mixed_terrains()
        map_id = np.array([2, 1], np.int32)
        x, start, goal = lc.points(name, B, 27, spread=lc.FOOTHOLD_SPREAD)
        Os = [Oracle(oracle_dict(cfg), height=maps[k], hcell=cell) for k in map_id]
    else:
        maps = map_id = None
        x, start, goal = lc.points(name, B, 27)
        Os = [O] * B
    assert cfg.terrain_mode == 1
    x = np.array([O.project_swings(row) for row in project_nodes(x, O.L, (~fx).astype(np.int32))])
    assert np.abs(x[:, (L.var_set == 1) & (L.var_is_vel == 0)]).max(axis=1).min() > 0.05      # not the trivial point
    out, kinds, sig, w = {}, {}, None, None
    for key in ((False, False),) + REDUCED:
        P = Planner(dataclasses.replace(cfg, reduce_base=key[0], reduce_swing=key[1]), max_batch=B)
        try:
            if maps is not None:
                P.set_heightfields(maps, cell)
            rk, vf, _ = P.structure()
            assert np.array_equal(vf == 0, fx)
            if sig is None:
                Ii = np.nonzero(rk == 2)[0]
                sig, w = np.zeros((B, P.m)), np.zeros((B, P.m))
                sig[:, Ii] = 10.0 ** rng.uniform(-2, 2, (B, len(Ii)))
                w[:, Ii] = rng.standard_normal((B, len(Ii)))
            P.debug_newton(start, goal, x, sig, w, map_id=map_id)
            dxr, res = P.debug_residual(B, refine=True)
        finally:
            P.close()
        out[key], kinds[key] = dxr, rk
        assert res.max() < 1e-10, (key, res)
    rk = kinds[(False, False)]
    free, E = np.nonzero(~fx)[0], np.nonzero(rk == 1)[0]
    for key in REDUCED:
        assert np.array_equal(kinds[key] == 2, rk == 2) and (kinds[key][E] != 1).any(), key
    full = out[(False, False)]
    entry = dict(problems=B, straight_line_guess_gate=1e-7, eps_dual=cfg.eps_dual, gap={}, gate={}, achieved={})
    fails = []
    for b in range(B):
        Jo, go = Os[b].jacobian(x[b]), Os[b].constraints(x[b])
        ref, r0 = _dense_step(Jo, go, free, E, Ii, sig[b], w[b], cfg.delta_x, np.full(len(E), cfg.eps_dual))
        scale = np.abs(ref).max()
        own = float(np.abs(full[b, free] - ref).max() / scale)
        entry["gpu_full_vs_dense"] = max(entry.get("gpu_full_vs_dense", 0.0), own)
        entry["dense_last_correction"] = max(entry.get("dense_last_correction", 0.0), r0)
        for key in REDUCED:
            k = "base" * key[0] + "+" * (key[0] and key[1]) + "swing" * key[1]
            eps = np.where(kinds[key][E] == 1, cfg.eps_dual, 1e-13)
            red, r1 = _dense_step(Jo, go, free, E, Ii, sig[b], w[b], cfg.delta_x, eps)
            gap = float(np.abs(red - ref).max() / scale)
            gate = max(lc.GATE_FACTOR * gap, own)
            achieved = float(np.abs(out[key][b] - full[b]).max() / scale)
            entry["dense_last_correction"] = max(entry["dense_last_correction"], r1)
            assert lc.GATE_FACTOR * max(r0, r1) <= gap, (k, r0, r1, gap)      # the dense solves are converged far below the gap they measure
            # (for the record, no gate: the reduced GPU step against the dense solve without the eliminated rows' regularisation)
            entry["gpu_reduced_vs_dense_reduced"] = max(entry.get("gpu_reduced_vs_dense_reduced", 0.0),
                                                        float(np.abs(out[key][b, free] - red).max() / scale))
            for what, v in (("gap", gap), ("gate", gate), ("achieved", achieved)):
                entry[what][k] = max(entry[what].get(k, 0.0), v)
            if achieved > gate:
                fails.append((b, k, achieved, gate))
            assert np.all(out[key][b, fx] == 0)
    lc.record("gpu_reduced_step_" + terrain, name, entry)
    assert not fails, fails
