"""The restatement of the dual infeasibility (oracle/duals.py) held on its own, without a GPU: test_gpu_steps.py and
test_gpu_report.py then hold dual_infeasibility() of csrc/kernels.hpp to it.

On every case of step_cases.DUAL_NAMES, with both reductions off and -- where the case's table entry runs the reduced system
-- under the three settings of step_cases.REDUCED_SETTINGS:
  * the basis Z has full column rank, and per group as many columns as the product's elimination order has variable entries;
  * the rows the reductions eliminate vanish on its range, in value and in their Jacobian;
  * the projections of a starting point leave its range alone;
  * with both reductions off the measure is the formula of test_gpu_report.py's full-system test;
and over the restatement's own runs of the cases:
  * discrimination: y dropped, z_l and z_u exchanged, Z replaced by the identity each move the value by more than ten times the
    gate the GPU test applies, on at least one state of every case;
  * coverage: every group of unknowns attains the maximum at least once, with the reductions off and with them on.
"""
import dataclasses

import numpy as np
import pytest
from scipy import sparse

import step_cases as stc
from oracle import duals, ipm, projection
from qtos_amd import capi

U = stc.U
FULL = (False, False)


def _settings(name):
    return (FULL,) + (stc.REDUCED_SETTINGS if stc.case(name).reduced else ())


SETTINGS = [(n, k) for n in stc.DUAL_NAMES for k in _settings(n)]
_ids = ["%s-%s" % (n, "full" if k == FULL else "+".join(w for w, on in zip(("base", "swing"), k) if on)) for n, k in SETTINGS]


def _free(c):
    return ipm.working_set(c.O, c.q[0])[0]


def _eliminated_rows(c, cfg):
    """The rows a reduction takes out of the KKT system: the acceleration-continuity rows of every junction but the first and
    the last interior one (those two are the double knots of base_knots: the spline is C1 there and the rows stay), and the
    swing rows."""
    L, rows = c.O.L, []
    if duals.base_is_reduced(L, cfg):
        nb = L.n_base_nodes - 1
        for off in (L.off_acc_lin, L.off_acc_ang):
            rows += [off + 3 * j + d for j in range(1, nb - 2) for d in range(3)]        # (row block j: the junction at node j + 1)
    if duals.swings_are_reduced(cfg):
        ends = list(L.off_swing[1:]) + [c.O.m]
        for e in range(4):
            rows += list(range(L.off_swing[e], ends[e]))
    return np.array(rows, int)


@pytest.mark.parametrize("name,key", SETTINGS, ids=_ids)
def test_the_basis_is_the_products_set_of_unknowns_and_the_eliminated_rows_vanish_on_it(name, key):
    c = stc.case(name)
    cfg = stc.setting(c, key)
    L, free = c.O.L, _free(c)
    Z, grp = stc.basis(name, key)
    n, p = Z.shape
    assert n == c.O.n and len(grp) == p
    fixed = np.setdiff1d(np.arange(n), free)
    assert Z[fixed].nnz == 0
    # full column rank: the unit columns stand on rows no other column touches, the rest has full rank as a dense matrix
    nnz = np.diff(Z.indptr)
    unit, other = np.nonzero(nnz == 1)[0], np.nonzero(nnz > 1)[0]
    assert (nnz >= 1).all() and (Z[:, unit].data == 1.0).all()
    unit_rows = Z[:, unit].indices
    assert len(np.unique(unit_rows)) == len(unit) and Z[unit_rows][:, other].nnz == 0
    if len(other):
        assert np.linalg.matrix_rank(Z[:, other].toarray()) == len(other)
    if key == FULL or not (duals.base_is_reduced(L, cfg) or duals.swings_are_reduced(cfg)):
        assert len(other) == 0 and np.array_equal(unit_rows, free)          # the identity on the free variables
    # the product's unknowns: solver variables are the node variables, then 6 x ncj coefficient ids (linear x, y, z, angular x, y, z)
    ncj = L.n_base_nodes + 4 if duals.base_is_reduced(L, cfg) else 0
    n_sol = n + 6 * ncj
    order = capi.analyze_order(cfg)
    d, _ = capi.analyze(cfg)
    order = order[order >= 0]
    assert len(order) == d.n_unknowns and len(np.unique(order)) == len(order) and order.max() < n_sol + c.O.m
    var = order[order < n_sol]
    want = np.bincount([duals.group_of_variable(L, v) if v < n else (v - n) // (3 * ncj) for v in var], minlength=4)
    assert np.array_equal(np.bincount(grp, minlength=4), want), (np.bincount(grp, minlength=4), want)
    # a point of the space: the straight-line guess (a spline of the space) with its swings on the rule, plus Z c
    rng = np.random.default_rng(11)
    vf = np.zeros(n, np.int32)
    vf[free] = 1
    xl, xh = c.O.var_bounds(c.q[0])
    x = c.O.initial_guess(c.q[0])
    if duals.swings_are_reduced(cfg):
        x = c.O.project_swings(x)
    x = x + Z @ (0.05 * rng.normal(size=p))
    assert np.array_equal(x[fixed], xl[fixed])
    rows = _eliminated_rows(c, cfg)
    if len(rows):
        g, J = c.O.constraints(x), c.O.jacobian(x)
        assert np.abs(g[rows]).max() <= stc.GATE_VALUE, np.abs(g[rows]).max()
        JZ = np.abs(J[rows] @ Z)
        assert (JZ.max(axis=1) <= stc.GATE_ENTRY * np.abs(J[rows]).sum(axis=1)).all(), JZ.max()
    # the projections leave the space alone
    scale = np.maximum(1.0, np.abs(x))
    if duals.base_is_reduced(L, cfg):
        assert (np.abs(projection.project_nodes(x, L, vf) - x) <= 64 * U * scale * L.n_base_nodes).all()
    if duals.swings_are_reduced(cfg):
        # (a mid node is a two-term combination of footholds with weights up to 1 / t_swing_avg, rounded once here and once in Z c)
        assert np.abs(c.O.project_swings(x) - x).max() <= 8 * U * scale.max() / min(1.0, cfg.t_swing_avg)


def _rows(c, R, S):
    """y, z_l, z_u of a state of the restatement's run, by constraint row."""
    y, zl, zu = np.zeros(c.O.m), np.zeros(c.O.m), np.zeros(c.O.m)
    y[R["E"]], zl[R["I"]], zu[R["I"]] = S["y"], S["zl"], S["zu"]
    return y, zl, zu


@pytest.mark.parametrize("name", stc.DUAL_NAMES)
def test_with_the_reductions_off_the_measure_is_the_formula_of_the_full_system_report_test(name):
    c = stc.case(name)
    Z, _ = stc.basis(name, FULL)
    R = stc.run(name, 0)
    free = R["free"]
    for S in R["states"]:
        y, zl, zu = _rows(c, R, S)
        J = c.O.jacobian(S["x"])
        val, col, info = duals.dual_infeasibility(J, Z, y, zl, zu)
        v = y + zu - zl
        du = np.abs(J[:, free].T @ v)                       # (test_final_measures_equal_a_float64_recomputation_on_the_full_system)
        assert abs(val - du.max()) <= ((info["terms"] + 4) * U * info["abs_terms"]).max()
        assert du[col] >= du.max() - 2 * ((info["terms"] + 4) * U * info["abs_terms"]).max()


_seen = {}


def _survey(name):
    """Per system ("full", "reduced") of a case: the groups that attain the maximum over the states of the restatement's run, and
    per mutation the largest move of the value in units of the state's gate."""
    if name in _seen:
        return _seen[name]
    c = stc.case(name)
    out = {}
    for system, key in (("full", FULL),) + ((("reduced", (True, True)),) if c.reduced else ()):
        Z, grp = stc.basis(name, key)
        ident = sparse.identity(c.O.n, format="csc")[:, _free(c)]
        groups, moves = set(), dict(y_dropped=0.0, z_exchanged=0.0, node_coordinates=0.0)
        # (the first problem's run: what it shows holds all the more over all of them; `groups` has a problem per group)
        for b in range(c.B if name == "groups" else 1):
            R = stc.run(name, b)
            for S in R["states"]:
                y, zl, zu = _rows(c, R, S)
                J = c.O.jacobian(S["x"])
                val, col, gate = stc.dual_measure(c, Z, S["x"], y, zl, zu, J)
                groups.add(duals.GROUPS[grp[col]])
                for what, args in (("y_dropped", (Z, 0 * y, zl, zu)), ("z_exchanged", (Z, y, zu, zl)), ("node_coordinates", (ident, y, zl, zu))):
                    if moves[what] <= 10.0:                 # (shown once is shown)
                        moves[what] = max(moves[what], abs(duals.dual_infeasibility(J, *args)[0] - val) / gate)
        out[system] = (groups, moves)
    _seen[name] = out
    return out


@pytest.mark.parametrize("name", stc.NAMES)
def test_three_wrong_measures_move_the_value_by_more_than_ten_gates_on_every_case(name):
    """What the GPU test would see of a kernel that left y out, exchanged z_l and z_u, or took the gradient in node
    coordinates.  The runs of step_cases.NAMES: `groups` has max_iter = 0 and no y (its states are state 0 only, where y = 0
    and exchanging the z only changes the sign of the gradient).  Node coordinates differ from solver coordinates on the
    reduced system only."""
    for system, (groups, moves) in _survey(name).items():
        for what, move in moves.items():
            if what == "node_coordinates" and system == "full":
                assert move == 0.0
                continue
            assert move > 10.0, (name, system, what, move)


def test_every_group_of_unknowns_attains_the_maximum_somewhere_in_the_full_and_in_the_reduced_system():
    """The kernel hands out the maximum only: an unknown that never attains it is not checked.  Over all cases and states
    every group attains it, separately for the two systems (`groups` is in step_cases for this)."""
    seen = {"full": {}, "reduced": {}}
    for name in stc.DUAL_NAMES:
        for system, (groups, _) in _survey(name).items():
            for g in groups:
                seen[system].setdefault(g, []).append(name)
    print("groups that attain the dual infeasibility:", seen)
    for system in seen:
        assert set(seen[system]) == set(duals.GROUPS), (system, seen[system])


@pytest.mark.parametrize("name", ["bilinear_1s", "bilinear_steps", "discard_trot", "bilinear_trot"])
def test_on_a_bilinear_map_a_stance_terrain_multiplier_is_eliminated_behind_its_foothold(name):
    """A multiplier eliminated in front of all its variables has the pivot -eps_dual and comes back as -(g + J dx) / eps_dual.
    With the one entry 1 of a flat or nearest-cell terrain row that is exact to rounding; with the bilinear map's slopes in J
    it turned an error of 7e-9 in the foothold's step into 2.7 in y (test_gpu_steps.py, item 9).  On a bilinear map the order
    therefore has every stance terrain row behind the last of its variables; elsewhere the rows stay at their node's time."""
    c = stc.case(name)
    L, n = c.O.L, c.O.n
    assert c.cfg_full.terrain_mode == 0
    J = c.O.jacobian(c.O.initial_guess(c.q[0]) + 0.01) != 0
    ends = list(L.off_terrain[1:]) + [L.off_dyn]
    found = 0
    for cfg, flat in ((c.cfg_full, False), (dataclasses.replace(c.cfg_full, terrain_mode=1), True)):
        order = capi.analyze_order(cfg)
        pos = {int(v): i for i, v in enumerate(order) if v >= 0}
        in_front = 0
        for e in range(4):
            for row in range(L.off_terrain[e], ends[e]):
                if n + row in pos:                          # (an equality row of the working set: a stance's)
                    mine = [pos[v] for v in np.nonzero(J[row])[0] if v in pos]
                    found += not flat
                    in_front += any(p > pos[n + row] for p in mine)
        assert (in_front > 0) == flat, (name, flat, in_front)
    assert found >= 4
