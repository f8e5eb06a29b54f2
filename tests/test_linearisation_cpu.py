"""The reference of test_gpu_linearisation.py held to something that shares no formula with it: the oracle's Jacobian against
Richardson-extrapolated difference quotients of the oracle's constraints, on every transcription of linearisation_cases.py at
the evaluation points the GPU tests use (noise 0.05 / 0.2 rad / 5 N), on flat ground and on a bilinear map; the case table
against the host analysis; the comparison itself.  No GPU.

The gate of a difference-quotient check is not a chosen number: 8 x max |R(h) - R(h/2)|, the quotients' own disagreement at
two step sizes (linearisation_cases.fd_check).  Floors, gates and achieved values are printed and kept where
QTOS_LINEARISATION_ACCURACY names a file."""
import dataclasses

import numpy as np
import pytest

import linearisation_cases as lc


def test_the_case_table_sits_on_the_paths_it_names(hip_lib):
    """Host analysis of the full system: the knot and range-of-motion counts of the table, more than one dynamics chunk
    (n_dyn_times > 128) and more than one range-of-motion chunk (4 n_rom_times > 512) for exactly the cases named for it."""
    from qtos_amd import capi
    for name in lc.NAMES:
        cfg, O, L = lc.case(name)
        d, _ = capi.analyze(lc.full(cfg))
        assert (d.n_vars, d.n_cons) == (O.n, O.m) and L.n_vars == O.n, name
        assert (d.n_dyn_times, d.n_rom_times) == lc.CASES[name][1:], name
        assert (d.n_dyn_times > lc.DYN_CHUNK_MAX) == (name in lc.TWO_DYN_CHUNKS), name
        assert (4 * d.n_rom_times > lc.ROM_CHUNK_MAX) == (name in lc.TWO_ROM_CHUNKS), name
        assert lc.COEF_IN_LDS[name] in (True, False, "not determined") and lc.lds_room(name) > 0
    d, _ = capi.analyze(lc.full(lc.case("two_dyn_chunks")[0]))
    assert d.n_dyn_times == 2 * 65                       # two chunks of 65: neither a whole number of waves
    assert 4 * lc.case("knots200_vel")[1].L.n_rom_times == 508      # just under one chunk


def test_points_differ_within_a_batch_and_leave_the_trivial_point():
    for name in ("walk", "trot"):
        cfg, O, L = lc.case(name)
        x, start, goal = lc.points(name, 3, 11)
        fx = lc.fixed(name)
        assert np.abs(x[0] - x[1])[~fx].min() > 0 and np.abs(x[1] - x[2])[~fx].min() > 0
        euler = (L.var_set == 1) & (L.var_is_vel == 0) & ~fx
        assert np.abs(x[:, euler]).max(axis=1).min() > 0.2
        x2, _, _ = lc.points(name, 3, 11)
        assert np.array_equal(x, x2)


@pytest.mark.parametrize("name", lc.NAMES)
def test_oracle_jacobian_against_richardson_differences_flat(name):
    cfg, O, L = lc.case(name)
    x, _, _ = lc.points(name, 1, 7)
    cols = lc.fd_columns(name)
    key = 2 * L.var_set + L.var_is_vel
    assert set(key[cols]) == set(key)                    # every variable set, values and derivatives
    assert len(cols) == (L.n_vars if L.n_vars <= lc.FD_ALL_COLUMNS_UP_TO else lc.FD_SAMPLE)
    floor, gate, achieved = lc.fd_check(O, x[0], cols, lc.FD_STEP)
    lc.record("oracle_fd_flat", name, dict(columns=len(cols), h=lc.FD_STEP, floor=floor, gate=gate, achieved=achieved))
    assert np.abs(O.jacobian(x[0])).max() > 1.0          # (the gate is an absolute one on entries of this size)
    assert achieved <= gate, "%s: |J - R(h)| = %.3e above the gate %.3e" % (name, achieved, gate)


@pytest.mark.parametrize("name", ["walk", "trot"])
def test_oracle_jacobian_against_richardson_differences_bilinear_terrain(name):
    """exp5_terrain() in bilinear mode, every foot-motion and force column.  A difference quotient across a kink of the
    bilinear surface is not a derivative: the point's seed is one that keeps every foot's x and y further than 2 h from a
    grid line, so no column is left out."""
    from oracle.oracle import Oracle, oracle_dict
    from qtos_amd import workloads
    cfg, _, L = lc.case(name)
    hxy, cell = workloads.exp5_terrain()
    O = Oracle(oracle_dict(dataclasses.replace(cfg, terrain_mode=0)), height=hxy, hcell=cell)
    x, _, _ = lc.points(name, 1, lc.TERRAIN_FD_SEED[name], spread=lc.FOOTHOLD_SPREAD)
    h = lc.FD_STEP_TERRAIN
    clearance = lc.grid_clearance(name, x[0], cell)
    assert clearance > 2 * h, clearance
    cols = np.nonzero(L.var_set >= 2)[0]
    # the footholds do stand on different heights: the terrain enters
    feet = lc.foot_motion(L) & (L.var_is_vel == 0)
    fx_, fy_ = x[0][feet & (L.var_dim == 0)], x[0][feet & (L.var_dim == 1)]
    assert len({O.terrain_height(a, b) for a, b in zip(fx_, fy_)}) > 3
    floor, gate, achieved = lc.fd_check(O, x[0], cols, h)
    lc.record("oracle_fd_bilinear", name, dict(columns=len(cols), h=h, grid_clearance=clearance, floor=floor, gate=gate, achieved=achieved))
    assert achieved <= gate, "%s: |J - R(h)| = %.3e above the gate %.3e" % (name, achieved, gate)


def test_the_comparison_sees_a_wrong_entry_and_a_filled_zero():
    cfg, O, L = lc.case("walk")
    x, _, _ = lc.points("walk", 1, 7)
    go, Jo = O.constraints(x[0]), O.jacobian(x[0])
    same = lc.compare(go, Jo, go, Jo, pattern=True)
    assert same == dict(values=0.0, entries=0.0, pattern_equal=True)
    r, c = [int(v[0]) for v in np.nonzero(Jo)]
    J = Jo.copy()
    J[r, c] += 10 * lc.GATE_ENTRY
    d = lc.compare(go, J, go, Jo, pattern=True)
    assert d["entries"] > lc.GATE_ENTRY and d["values"] == 0.0 and d["pattern_equal"]
    r0, c0 = [int(v[0]) for v in np.nonzero(Jo == 0)]
    J = Jo.copy()
    J[r0, c0] = 1e-300
    d = lc.compare(go, J, go, Jo, pattern=True)
    assert d["entries"] < lc.GATE_ENTRY and not d["pattern_equal"]
    g = go.copy()
    g[-1] += 10 * lc.GATE_VALUE
    assert lc.compare(g, Jo, go, Jo)["values"] > lc.GATE_VALUE
    # the masks of the GPU tests
    rk = np.ones(O.m, int)
    rk[3] = 0
    Jm = lc.mask_jacobian(Jo, lc.fixed("walk"), rk)
    assert not Jm[:, lc.fixed("walk")].any() and not Jm[3].any() and np.array_equal(Jm[4][~lc.fixed("walk")], Jo[4][~lc.fixed("walk")])
