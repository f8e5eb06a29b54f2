"""What the force-QP tests share (tests/test_force_qp_cpu.py, tests/test_gpu_force_qp.py): the cases, a dense longdouble restatement
of a row's problem that is independent of the rule's structured formulas, the certificate, the enumeration of active sets, the
gates and the recorder.

Cases, at hz = 50, so that a 5 s plan is 251 rows (plans: tests/force_fit_cases.py; the rule reads nodes as data):

  trot    the reference_compat trot, mu 0.2 and f_max 16 N.  The trot walks straight: its fitted forces never leave a pyramid of
          mu 0.2 (1 row of 251 does, one with f_z = 0), so mu 0.2 alone does not meet the condition of 5 % below; its two-stance
          rows carry up to 23 N per foot, and the cap of 16 N limits them.
  walk    the golden walk, f_max 12 N (its largest f_z is 18.3 N)
  ledge   the walk onto the ledges of exp_5, mu 0.3, terrain_mode 0 (bilinear) on the ledges plus a smooth swell of 1.5 cm, so
          that the slopes under the feet are not zero (up to 0.12); the plan was solved on the ledges alone
  synth   69 rows of the trot (both diagonal pairs, four feet) and of the walk (three feet) at mu 0.15 and f_max 14 N, at the rate
          of 14.03 rows per second from row 1, so that their times are no multiples of anything a phase lasts: every stance
          pattern on a limit.  (The kernel takes rows as first_row and hz, not as a list of times, so the rule takes them so too.)

Gates.  The float64 rule's distance from the longdouble rule over the rows of all cases is the floor of a column group
(group_floors); a GPU gate is 8 x that floor per column group (the margin of tests/plan_check_cases.py), never taken from the kernel's output.  Columns 1 and 2 of the solve's
table (the complementarity and stationarity residuals the iteration stopped at) are residuals of rounding and, where the step
counts differ by one, of another iterate: they are held to the thresholds they were stopped by, CTOL and RTOL (1 + |q|inf)."""
import dataclasses
import itertools
import json
import os

import numpy as np

import force_fit_cases as ffc

LD, F64 = np.longdouble, np.float64
HZ = 50.0
T0 = 3.756
TOL = (1e-3, 1e-2, 5.0, 1e-2)
GROUPS = {"f_qp": slice(1, 13), "res_ang": slice(13, 16), "res_lin": slice(16, 19), "change": slice(19, 20), "tau": slice(20, 32)}
QGROUPS = {"slack": slice(3, 4), "mult": slice(4, 5), "limited": slice(5, 6), "cost": slice(6, 7)}
MARGIN = 8.0


def swell(height, cell):
    """The heightfield plus a smooth swell of 1.5 cm (slopes up to 0.12)."""
    nx, ny = height.shape
    x, y = np.meshgrid(np.arange(nx) * cell, np.arange(ny) * cell, indexing="ij")
    return height + 0.015 * np.sin(7.0 * x + 0.3) * np.cos(5.0 * y - 0.2)


class QpCase:
    """cfg, L, nodes, terrain, the QpParams, and the rows: n rows from row `first` at the rate hz."""

    def __init__(self, name):
        from qtos_amd import force_qp as fq
        self.name, self.hz, self.first = name, HZ, 0
        if name == "trot":
            P, kw = ffc.plan("trot"), dict(mu=0.2, f_max=16.0)
        elif name == "walk":
            P, kw = ffc.plan("walk"), dict(f_max=12.0)
        elif name == "ledge":
            P, kw = ffc.plan("exp5"), dict(mu=0.3)
        elif name == "synth_trot":
            P, kw = ffc.plan("trot"), dict(mu=0.15, f_max=14.0)
        elif name == "synth_walk":
            P, kw = ffc.plan("walk"), dict(mu=0.15, f_max=14.0)
        else:
            raise KeyError(name)
        self.cfg, self.L, self.x, self.terrain = P.cfg, P.L, P.x, P.terrain
        if name == "ledge":
            self.cfg = dataclasses.replace(P.cfg, terrain_mode=0)
            h, cell, x0, y0 = P.terrain
            self.terrain = (swell(np.asarray(h, F64), cell), cell, x0, y0)
        self.n = int(round(self.cfg.duration * HZ)) + 1
        if name.startswith("synth"):
            self.hz, self.first, self.n = 14.03, 1, 69                              # 0.0713 .. 4.918 s
        self.qp = fq.qp_params(self.cfg, **kw)
        self._rows = {}

    def rows(self, dtype, joint=None):
        """(rows, qrows, status, detail) of the rule in dtype, computed once (and once more with joint rows [n, 37])."""
        from qtos_amd import force_qp as fq
        key = (dtype, joint is not None)
        if key not in self._rows:
            out = fq.qp_rows(self.L, self.x, T0, self.hz, self.first, self.n, self.cfg, self.qp, terrain=self.terrain, joint=joint, dtype=dtype,
                             detail=True)
            for a in out[:3]:
                a.setflags(write=False)
            self._rows[key] = out
        return self._rows[key]


NAMES = ("trot", "walk", "ledge", "synth_trot", "synth_walk")
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = QpCase(name)
    return _cases[name]


def dist(a, b):
    a, b = np.asarray(a, LD), np.asarray(b, LD)
    return float(np.abs(a - b).max()) if a.size else 0.0


def guard(c):
    """(band, in_band [n]): the band is 8 x the float64 floor of the fit's largest limit-row value (the path switch), by the
    longdouble rule; in_band: the rows whose longdouble value lies within the band of 0."""
    v64, vld = c.rows(F64)[3]["fit_value"], c.rows(LD)[3]["fit_value"]
    fin = np.isfinite(vld)
    band = MARGIN * dist(v64[fin], vld[fin])
    return band, fin & (np.abs(vld) <= band)


def floors(c, keep, joint=None):
    """{group: float64 floor} of a case over the rows `keep`."""
    (o64, q64, _, _), (old, qld, _, _) = c.rows(F64, joint), c.rows(LD, joint)
    out = {g: dist(o64[keep][:, s], old[keep][:, s]) for g, s in GROUPS.items() if g != "tau" or joint is not None}
    out.update({g: dist(q64[keep][:, s], qld[keep][:, s]) for g, s in QGROUPS.items()})
    return out


_group_floors = {}


def group_floors(ledge_joint=None):
    """{group: the float64 floor over the rows of ALL cases outside their guard bands}: what a GPU gate is 8 x of.  One case's
    rows are too few to show the float64 rule's error: the 69 rows of synth_walk put f_qp's floor at 7.1e-12 N where the 251
    rows of the walk they are taken from put it at 2.8e-10 N.  ledge_joint: the ledge case's joint rows [n, 37], for the group tau."""
    key = ledge_joint is not None
    if key not in _group_floors:
        out = {}
        for name in NAMES:
            c = case(name)
            fl = floors(c, ~guard(c)[1], ledge_joint if name == "ledge" else None)
            for g, v in fl.items():
                out[g] = max(out.get(g, 0.0), v)
        _group_floors[key] = out
    return _group_floors[key]


# ---- a row's problem, dense, in longdouble, from the detail's d, w, stance, rho_s, c, slopes and f alone --------------------------
def skew(d):
    return np.array([[0, -d[2], d[1]], [d[2], 0, -d[0]], [-d[1], d[0], 0]], LD)


class Dense:
    """Row k of a detail: A [6, 3n], H, q, G [6n, 3n], hf = h - G f, feet the stance feet; objective(x) with its constant."""

    def __init__(self, D, k, qp):
        self.feet = [e for e in range(4) if D["stance"][k, e]]
        n = len(self.feet)
        self.n = n
        A, G, hf = np.zeros((6, 3 * n), LD), np.zeros((6 * n, 3 * n), LD), np.zeros(6 * n, LD)
        Winv = np.zeros(3 * n, LD)
        mu, fmax = LD(qp.mu), LD(qp.f_max)
        for i, e in enumerate(self.feet):
            A[0:3, 3 * i:3 * i + 3], A[3:6, 3 * i:3 * i + 3] = skew(np.asarray(D["d"][k, e], LD)), np.eye(3, dtype=LD)
            hx, hy = LD(D["slopes"][k, e, 0]), LD(D["slopes"][k, e, 1])
            nn, t1, t2 = np.array([-hx, -hy, 1], LD), np.array([1, 0, hx], LD), np.array([0, 1, hy], LD)
            nn, t1, t2 = nn / np.sqrt((nn * nn).sum()), t1 / np.sqrt((t1 * t1).sum()), t2 / np.sqrt((t2 * t2).sum())
            Ge = np.stack([-nn, nn, t1 - mu * nn, -(t1 + mu * nn), t2 - mu * nn, -(t2 + mu * nn)])
            G[6 * i:6 * i + 6, 3 * i:3 * i + 3] = Ge
            he = np.array([0, fmax, 0, 0, 0, 0], LD)
            hf[6 * i:6 * i + 6] = he - Ge @ np.asarray(D["f"][k, e], LD)
            Winv[3 * i:3 * i + 3] = LD(1) / LD(D["w"][k, e])
        self.A, self.G, self.hf, self.c = A, G, hf, LD(qp.damping) * n
        self.rho = np.asarray(D["rho_s"][k], LD)
        self.H = A.T @ A + np.diag(self.c * Winv)
        self.q = -(A.T @ self.rho)
        self.Winv = Winv

    def x_of(self, forces, D, k):
        """x [3n] of a row of forces [12] (any float type): f_qp - f over the stance feet, in longdouble."""
        f = np.asarray(forces, LD).reshape(4, 3)
        return np.concatenate([f[e] - np.asarray(D["f"][k, e], LD) for e in self.feet])

    def objective(self, x):
        r = self.rho - self.A @ x
        return LD(0.5) * (r @ r) + LD(0.5) * self.c * ((x * x) @ self.Winv)


def solve_ld(M, b):
    """x of M x = b by Gaussian elimination with partial pivoting in longdouble, batched: M [m, N, N], b [m, N].  Returns (x,
    smallest |pivot| / largest |entry| per system): numpy.linalg has no longdouble."""
    M, b = np.array(M, LD), np.array(b, LD)
    m, N = b.shape
    scale = np.abs(M).reshape(m, -1).max(axis=1)
    piv_min = np.full(m, np.inf, LD)
    ar = np.arange(m)
    for j in range(N):
        p = j + np.argmax(np.abs(M[:, j:, j]), axis=1)
        Mj, Mp = M[ar, j].copy(), M[ar, p].copy()
        M[ar, j], M[ar, p] = Mp, Mj
        bj, bp = b[ar, j].copy(), b[ar, p].copy()
        b[ar, j], b[ar, p] = bp, bj
        piv = M[:, j, j]
        piv_min = np.minimum(piv_min, np.abs(piv))
        safe = np.where(piv == 0, LD(1), piv)
        fac = M[:, j + 1:, j] / safe[:, None]
        M[:, j + 1:, :] -= fac[:, :, None] * M[:, j, :][:, None, :]
        b[:, j + 1:] -= fac * b[:, j][:, None]
    x = np.zeros((m, N), LD)
    for i in range(N - 1, -1, -1):
        safe = np.where(M[:, i, i] == 0, LD(1), M[:, i, i])
        x[:, i] = (b[:, i] - (M[:, i, i + 1:] * x[:, i + 1:]).sum(axis=1)) / safe
    return x, piv_min / np.where(scale > 0, scale, LD(1))


def certificate(P, x, mu_end):
    """From x alone, in longdouble: (smallest slack, |H x + q + G^T (mu_end / s)|inf, objective(x) - dual objective at z = mu_end / s)."""
    s = P.hf - P.G @ x
    z = LD(mu_end) / s
    r = P.H @ x + P.q + P.G.T @ z
    # the dual function at z: min over x' of the Lagrangian, attained where H x' = -(q + G^T z)
    xs, _ = solve_ld(P.H[None], (-(P.q + P.G.T @ z))[None])
    xs = xs[0]
    dual = P.objective(xs) + z @ (P.G @ xs - P.hf)
    return float(s.min()), float(np.abs(r).max()), float(P.objective(x) - dual)


def enumerate_optimum(P):
    """The optimum of a two-stance row's QP by enumeration of its 4096 active sets: each an equality-constrained solve in
    longdouble; the optimum is the objective of the feasible KKT point (x feasible, multipliers >= 0).  Returns (optimum, number
    of feasible KKT points found)."""
    assert P.n == 2
    nv, nc = 6, 12
    masks = np.array(list(itertools.product((0, 1), repeat=nc)), LD)               # [4096, 12]
    m = len(masks)
    K = np.zeros((m, nv + nc, nv + nc), LD)
    K[:, :nv, :nv] = P.H[None]
    K[:, :nv, nv:] = P.G.T[None] * masks[:, None, :]
    K[:, nv:, :nv] = P.G[None] * masks[:, :, None]
    K[:, nv + np.arange(nc), nv + np.arange(nc)] = 1 - masks
    rhs = np.concatenate([np.broadcast_to(-P.q, (m, nv)), P.hf[None] * masks], axis=1)
    sol, piv = solve_ld(K, rhs)
    x, lam = sol[:, :nv], sol[:, nv:]
    viol = (x @ P.G.T - P.hf[None]).max(axis=1)
    ok = (piv > 1e-13) & (viol <= 1e-11) & (lam.min(axis=1) >= -1e-11)
    assert ok.any()
    obj = np.array([P.objective(xx) for xx in x[ok]], LD)
    return obj.min(), int(ok.sum()), float(obj.max() - obj.min())


def record(name, entry):
    print("force qp accuracy [%s]: %s" % (name, json.dumps(entry)))
    path = os.environ.get("QTOS_FORCE_QP_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
