"""The dual infeasibility of an interior-point iterate, restated in plain numpy (TEST INFRASTRUCTURE ONLY).

What dual_infeasibility() of csrc/kernels.hpp hands to k_start, k_step and k_report: the largest entry of the gradient of
the Lagrangian, J' (y + z_u - z_l), taken per UNKNOWN OF THE KKT SYSTEM -- with the reduced base those are the coefficients
of the clamped cubic B-spline of oracle/projection.py, with the reduced swings the footholds carried through the swing rule,
and every other free node variable as it is.  This file states the unknowns as a matrix Z (node variables x unknowns) from
the spline space and the oracle's swing rule alone, and the measure as max_p |Z[:, p]' J' (y + z_u - z_l)| with the oracle's
dense Jacobian: no index list, order or table of the product enters.  Sums in np.longdouble.
"""
import numpy as np
from scipy import sparse

from .projection import base_knots, nodes_of_coefficients

GROUPS = ("base linear", "base angular", "foot motion", "force")


def base_is_reduced(L, cfg):
    """Whether reduce_base takes effect (at least 20 base polynomials, all of one duration -- with a shorter last
    polynomial the straight-line guess is no spline of the coefficients' space and the full system is kept)."""
    nb = L.n_base_nodes - 1
    return bool(cfg.reduce_base) and nb >= 20 and abs(L.T - nb * cfg.dt_base) <= 1e-9 * L.T


def swings_are_reduced(cfg):
    """Whether reduce_swing takes effect: nearest-cell terrain only (oracle_dict states the same rule)."""
    return bool(cfg.reduce_swing) and cfg.terrain_mode == 1


def group_of_variable(L, v):
    """The group (index into GROUPS) of node variable v."""
    return 0 if v < L.off_ang else 1 if v < L.off_eem[0] else 2 if v < L.off_eef[0] else 3


def solver_basis(O, L, cfg, free):
    """(Z, groups): Z [n_vars x unknowns] (scipy CSC) whose columns are the KKT system's variable unknowns expressed in node
    variables -- zero on the fixed ones --, and per column the index into GROUPS.  free: the indices of the free variables.

      reduce_base: per base dimension (linear and angular) the node values and velocities of the unit coefficient vectors of
        the clamped cubic B-spline on base_knots().  A fixed end value takes the end coefficient away (p(t_0) = c_0); a fixed
        end derivative ties its neighbour to it (p'(t_0) = 3 (c_1 - c_0) / h: c_1 moves with c_0, or not at all where c_0 is
        gone); likewise at the end.
      reduce_swing: a foothold's x or y carried through the oracle's swing rule (Oracle.project_swings of the unit vector:
        the rule is linear and homogeneous); the variables the rule sets are no unknowns.
      every other free variable: a unit column."""
    n = O.n
    is_free = np.zeros(n, bool)
    is_free[np.asarray(free)] = True
    cols, groups = [], []
    taken = np.zeros(n, bool)                              # variables that are no unknowns of their own
    if base_is_reduced(L, cfg):
        nb = L.n_base_nodes - 1
        knots, t = base_knots(nb, L.T)
        ncj = len(knots) - 4
        unit = np.eye(ncj)
        nodes = [nodes_of_coefficients(knots, unit[j], t) for j in range(ncj)]
        for which, off in enumerate((L.off_lin, L.off_ang)):
            for d in range(3):
                ip = off + 6 * np.arange(nb + 1) + d
                iv = ip + 3
                taken[ip] = taken[iv] = True
                N = np.zeros((n, ncj))
                for j in range(ncj):
                    N[ip, j], N[iv, j] = nodes[j]
                keep = np.ones(ncj, bool)
                for jp, jv, node in ((0, 1, 0), (ncj - 1, ncj - 2, nb)):
                    if not is_free[iv[node]]:
                        N[:, jp] += N[:, jv]
                        keep[jv] = False
                    if not is_free[ip[node]]:
                        keep[jp] = False
                for j in np.nonzero(keep)[0]:
                    assert np.abs(N[~is_free, j]).max(initial=0.0) < 1e-12      # an unknown moves no fixed variable
                    N[~is_free, j] = 0.0
                    cols.append(sparse.csc_matrix(N[:, j][:, None]))
                    groups.append(which)
    if swings_are_reduced(cfg):
        probe = np.random.default_rng(0).random(n) + 1.0
        taken |= O.project_swings(probe) != probe
        assert not (taken & ~is_free)[L.off_eem[0]:].any()
    for v in np.nonzero(is_free & ~taken)[0]:
        e = sparse.csc_matrix(([1.0], ([v], [0])), shape=(n, 1))
        if swings_are_reduced(cfg) and L.off_eem[0] <= v < L.off_eef[0]:
            e = np.zeros(n)
            e[v] = 1.0
            e = sparse.csc_matrix(O.project_swings(e)[:, None])
        cols.append(e)
        groups.append(group_of_variable(L, v))
    return sparse.hstack(cols, format="csc"), np.array(groups)


def _column_sums(M, x):
    """sum_i M[i, p] x[i] per column p of the CSC matrix M, in np.longdouble (x: one np.longdouble per row)."""
    prod = np.append(M.data.astype(np.longdouble) * x[M.indices], np.longdouble(0))
    out = np.add.reduceat(prod, np.minimum(M.indptr[:-1], len(prod) - 1))
    out[M.indptr[1:] == M.indptr[:-1]] = 0                 # (reduceat hands an empty segment the element behind it)
    return out


def lagrangian_gradient(J, y, zl, zu):
    """Per node variable, with v = y + z_u - z_l by constraint row and in np.longdouble: (J' v, |J|' |v|, the number of
    entries with v != 0, the sum of |v| over the entries)."""
    v = y.astype(np.longdouble) + zu.astype(np.longdouble) - zl.astype(np.longdouble)
    Jc = sparse.csc_matrix(J)
    Ja, Jp = abs(Jc), Jc.copy()
    Jp.data = np.ones_like(Jp.data)
    return _column_sums(Jc, v), _column_sums(Ja, np.abs(v)), _column_sums(Jp, (v != 0).astype(np.longdouble)), _column_sums(Jp, np.abs(v))


def dual_infeasibility(J, Z, y, zl, zu):
    """(value, attaining column, per-column figures) of max_p |Z[:, p]' J' (y + z_u - z_l)|; J all rows x all variables, y,
    z_l, z_u by constraint row.  The figures, for a rounding bound: abs_terms, the sum of the absolute terms sum |Z| |J| |v|;
    terms, their number; weight, sum |Z| |v| over the Jacobian entries that enter (what an error per entry weighs); values."""
    r, a, cnt, w = lagrangian_gradient(J, y, zl, zu)
    Z = sparse.csc_matrix(Z)
    Za, Zp = abs(Z), Z.copy()
    Zp.data = np.ones_like(Zp.data)
    val = np.abs(_column_sums(Z, r))
    k = int(np.argmax(val))
    return float(val[k]), k, dict(abs_terms=_column_sums(Za, a).astype(np.float64), terms=np.rint(_column_sums(Zp, cnt).astype(np.float64)).astype(np.int64),
                                  weight=_column_sums(Za, w).astype(np.float64), values=val.astype(np.float64))
