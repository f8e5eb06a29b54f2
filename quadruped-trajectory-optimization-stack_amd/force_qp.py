"""Force QP: the force fit inside the friction pyramid.  The rule of k_force_qp (qtos_force_qp*, include/qtos_planner.h) stated in
numpy, built on force_fit.py, which it leaves as it is.

force_fit.fit_rows gives every row the forces that supply the wrench the planned motion needs; nothing keeps them inside what a
foot can do.  Here the same least-squares objective is minimised under the NLP's five force rows of every stance foot, written
as six rows G_e f_e <= h_e with the terrain basis (n, t1, t2) at the foot (plan_check.force_rows' basis):

    -n.f <= 0     n.f <= f_max     (t1 - mu n).f <= 0     -(t1 + mu n).f <= 0     (t2 - mu n).f <= 0     -(t2 + mu n).f <= 0

mu and f_max are parameters of the call (None: the planner's friction and force_limit).  Per row, in x = (df_e), e in S, with
c = damping n and everything up to M, y and df_fit taken from force_fit.py's functions unchanged:

    minimise   1/2 |rho~ - sum_S A~_e df_e|^2 + 1/2 c sum_S |df_e|^2 / w_e      subject to   G_e (f_e + df_e) <= h_e,  e in S

Without the limits the minimiser is the fit's df_e = w_e A~_e^T y: the fit is the ridge solution of this objective.

1. Fit path.  Where every limit row of the fit's forces f + df_fit has a value G f - h <= 0, the row is fit_rows' row, to the bit.
2. Limited path.  Otherwise the result is DEFINED as the central point of the barrier problem at the fixed weight mu_end: the
   unique minimiser of the objective - mu_end sum log(h - G f).  With damping 1e-6 the objective is flat along the internal
   forces, so "the optimum to a stopping tolerance" is no well-defined number; the central point is a smooth function of the
   data, strictly feasible, and suboptimal by at most 6 n mu_end (the duality gap of a central point).  It is computed by the
   feasible-start primal-dual iteration below.
3. A row without a stance foot, a swing foot and a non-finite row behave as in the fit (nothing fitted, the plan's force to the
   bit, NaN in columns 13 .. 19 with NONFINITE).  A row that reaches the cap of max_iter steps keeps its last iterate, which is
   feasible, and says so (CAP).

The order of the operations (only +, -, x, /, sqrt and comparisons; a sum a + b + c is (a + b) + c, feet in the order FL FR HL
HR, limit rows in the order above), the one the kernel runs with contraction off:

  basis      bn = (-hx, -hy, 1) / |.|, b1 = (1, 0, hx) / |.|, b2 = (0, 1, hy) / |.|, |v| = sqrt((v0 v0 + v1 v1) + v2 v2)
  G v        a = bn.v, b = b1.v, c2 = b2.v, u.v = (u0 v0 + u1 v1) + u2 v2; ma = mu a;
             (-a, a, b - ma, -(b + ma), c2 - ma, -(c2 + ma))
  G^T y      al = (y1 - y0) - mu (((y2 + y3) + y4) + y5), be = y2 - y3, ga = y4 - y5;  (bn_i al + b1_i be) + b2_i ga
  H          blocks of 3 x 3 over the feet: for stance feet e >= e', H[3e+i, 3e'+j] = (dd + 1) [i = j] - d_e'[i] d_e[j] with
             dd = d_e . d_e'; on the diagonal blocks c / w_e is added to the diagonal entries last; a swing foot has an identity
             block and zeros elsewhere (as fit_rows pads rows without stance)
  grad       r~ = rho~ - sum_S (d_e x x_e, x_e), foot after foot; grad_e = (c / w_e) x_e - ((r~_ang x d_e) + r~_lin); 0 for a swing foot
  q          the gradient at x = 0: -((rho~_ang x d_e) + rho~_lin)
  start      g_e = bn.f_e; gam_e = min(max(g_e, min(1, f_max / 4)), f_max / 2); x_int_e = bn gam_e - f_e;
             s_int = h - G (f + x_int); dir = x_fit - x_int; ds = -G dir; theta = min(1, 0.9 min over ds < 0 of s_int / -ds);
             x = x_int + theta dir; s = h - G (f + x); z = 1 / s
  loop       steps = 0, 1, ...:  m = 6 n; mu_k = (sum s z) / m; r_d = grad + G^T z; comp = max |s z - mu_end| / mu_end;
             stop where comp <= CTOL and |r_d|inf <= RTOL (1 + |q|inf); CAP where steps = max_iter; else one step:
    K        H + G^T diag(z / s) G, per foot B^T C B with D = z / s, S = ((D2 + D3) + D4) + D5, C_nn = (D0 + D1) + (mu mu) S,
             C_n1 = mu (D3 - D2), C_n2 = mu (D5 - D4), C_11 = D2 + D3, C_22 = D4 + D5; T_n = (C_nn bn + C_n1 b1) + C_n2 b2,
             T_1 = C_n1 bn + C_11 b1, T_2 = C_n2 bn + C_22 b2; block_ij = (bn_i T_n,j + b1_i T_1,j) + b2_i T_2,j, i >= j, added to
             H's diagonal block of a stance foot
    factor   the unpivoted Cholesky of force_fit.cholesky_solve at size 12, one factorisation for both solves
    predict  where mu_k > 10 mu_end: K dx_a = -grad; ds_a = -G dx_a; dz_a = -z - D ds_a; al_a = min(1, ratio tests on s and z);
             mu_a = (sum (s + al_a ds_a)(z + al_a dz_a)) / m; sigma = (mu_a / mu_k)^3; target = max(sigma mu_k, mu_end);
             rc = (target - s z) - ds_a dz_a.   Else (centering): target = mu_end, rc = target - s z
    solve    K dx = -(r_d + G^T (rc / s)); ds = -G dx; dz = rc / s - D ds
    length   al = min(1, 0.99 min(ratio test on s, ratio test on z)), ratio test: min over d < 0 of v / -d; x, s, z += al d
  Every iterate is strictly feasible (ds = -G dx: there is never a primal residual).

CTOL = 1e-10 and RTOL = 1e-9.  Newton converges quadratically at the end: one more step takes comp from 1e-5 or so to 1e-10 and
below, and float64 holds the CARRIED s and z of the iteration to 1e-16 relative, so 1e-10 is reached without a step spent on
rounding noise (no row of the test cases needs more than one step over what CTOL = 1e-6 needs).  It leaves CTOL x the largest
multiplier, 1e-10 x 50 N, in the barrier's stationarity residual -- below what a float64 TABLE can certify at all: the slack of
an active row is mu_end / z = 1e-7 N and less next to forces of 10 N, known to 1e-8 .. 1e-7 relative from the forces alone, which
is 1e-7 .. 1e-6 N of residual.  A tighter CTOL buys nothing that the forces can show.

Outputs per row: the fit's 32 columns (force_fit.py) with f_qp in place of f_fit -- columns 13 .. 18 are rho - A df_qp, column 19
sqrt(sum |f_qp - f|^2), columns 20 .. 31 tau_ff from f_qp; an 8-column table of the solve (QP_COLS):

   0   steps taken (0 on the fit path)
   1   max |s z - mu_end| / mu_end                       2   |r_d|inf                                   [N]
   3   the smallest slack over the stance feet  [N]      4   the largest multiplier
   5   sqrt(sum |f_qp - f_fit|^2)               [N]      6   objective(f_qp) - objective(f_fit), >= 0: what the limits cost  [N^2]
   7   the number of limit rows with slack <= act_tol

(on the fit path columns 1, 2, 4, 5, 6 are 0 and 3, 7 come from the fit's slacks; a row without stance has zeros; a non-finite
row NaN in 1 .. 6), and a status word: bits 0 .. 2 the fit's (NO_STANCE, TWO_STANCE, NONFINITE), bit 3 + e (ACTIVE << e) foot e
has a limit row with slack <= act_tol, bit 7 (CAP) the cap was reached, bit 8 (LIMITED) the row took the limited path.
Column 6 is formed as grad_fit . D + 1/2 (|A~ D|^2 + c sum |D_e|^2 / w_e), D = x - x_fit, which does not cancel.

The summary has four families with plan_check.summarise's semantics and accumulate's merge: res_ang max |13 .. 15|, res_lin
max |16 .. 18|, change column 19 and limited, column 5 of the solve's table.  It is a function of the two tables alone.
"""
import numpy as np

from . import force_fit as ff
from . import joints
from . import plan_check as pc

NEE = 4
COLS, QP_COLS = ff.COLS, 8
FAMILIES = ("res_ang", "res_lin", "change", "limited")
UNITS = ("N m", "N", "N", "N")
SUMMARY = pc.SUMMARY
ACCUMULATE = 1
NO_STANCE, TWO_STANCE, NONFINITE, ACTIVE, CAP, LIMITED = 1, 2, 4, 8, 128, 256
QP_TOL = (1e-3, 1e-2, 5.0, 1e-2)                 # the default tol per family: N m, N, N, N
CTOL, RTOL = 1e-10, 1e-9
MAX_ITER = 25


class QpParams(ff.FitParams):
    """FitParams and the limits: mu, f_max (None: the planner's friction and force_limit, filled in by qp_params), the barrier
    weight mu_end [N^2], act_tol [N] and max_iter (1 .. 25).  capi.QtosForceQp has the same field names and is taken as well."""

    def __init__(self, mu, f_max, mu_end=1e-6, act_tol=1e-3, max_iter=MAX_ITER, **kw):
        super().__init__(**kw)
        self.mu, self.f_max, self.mu_end, self.act_tol, self.max_iter = float(mu), float(f_max), float(mu_end), float(act_tol), int(max_iter)
        if not self.mu > 0 or not self.f_max > 0 or not self.mu_end > 0 or not (1 <= self.max_iter <= MAX_ITER) or self.act_tol != self.act_tol:
            raise ValueError("mu > 0, f_max > 0, mu_end > 0, max_iter in 1 .. 25, act_tol a number")


def qp_params(cfg=None, mu=None, f_max=None, **kw):
    """The QpParams of a planner configuration: mu and f_max default to cfg's friction and force_limit (cfg None: PlannerConfig's)."""
    if mu is None or f_max is None:
        if cfg is None:
            from .config import PlannerConfig
            cfg = PlannerConfig()
        mu = cfg.friction if mu is None else mu
        f_max = cfg.force_limit if f_max is None else f_max
    return QpParams(mu, f_max, **kw)


def _dot(u, v):
    return (u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1]) + u[:, 2] * v[:, 2]


def basis(hx, hy, dtype):
    """[n, 3, 3]: bn, b1, b2 of the slopes hx, hy [n]."""
    one, zero = np.ones(len(hx), dtype), np.zeros(len(hx), dtype)
    out = np.empty((len(hx), 3, 3), dtype)
    for a, v in enumerate(((-hx, -hy, one), (one, zero, hx), (zero, one, hy))):
        nn = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        out[:, a, 0], out[:, a, 1], out[:, a, 2] = v[0] / nn, v[1] / nn, v[2] / nn
    return out


def g_mul(B, mu, v):
    """G v [n, 6] of one foot: B [n, 3, 3], v [n, 3]."""
    a, b, c2 = _dot(B[:, 0], v), _dot(B[:, 1], v), _dot(B[:, 2], v)
    ma = mu * a
    return np.stack([-a, a, b - ma, -(b + ma), c2 - ma, -(c2 + ma)], axis=1)


def gt_mul(B, mu, y):
    """G^T y [n, 3] of one foot: y [n, 6]."""
    al = (y[:, 1] - y[:, 0]) - mu * (((y[:, 2] + y[:, 3]) + y[:, 4]) + y[:, 5])
    be, ga = y[:, 2] - y[:, 3], y[:, 4] - y[:, 5]
    return np.stack([(B[:, 0, i] * al + B[:, 1, i] * be) + B[:, 2, i] * ga for i in range(3)], axis=1)


def hessian(d, w, stance, c, dtype):
    """H [n, 12, 12], the lower triangle filled (the rest zero)."""
    n = len(d)
    H = np.zeros((n, 12, 12), dtype)
    one = dtype(1)
    for e in range(NEE):
        for e2 in range(e + 1):
            both = stance[:, e] & stance[:, e2]
            dd = _dot(d[:, e], d[:, e2])
            for i in range(3):
                for j in range(3):
                    if e == e2 and j > i:
                        continue
                    v = -(d[:, e2, i] * d[:, e, j])
                    if i == j:
                        v = (dd + one) - d[:, e2, i] * d[:, e, j]
                        if e == e2:
                            v = v + c / w[:, e]
                    pad = one if (e == e2 and i == j) else dtype(0)
                    H[:, 3 * e + i, 3 * e2 + j] = np.where(both, v, pad)
    return H


def cholesky(K, dtype):
    """L [n, N, N] of K's lower triangle, unpivoted, force_fit.cholesky_solve's order."""
    n, N = K.shape[0], K.shape[1]
    L = np.zeros((n, N, N), dtype)
    for j in range(N):
        acc = K[:, j, j].copy()
        for k in range(j):
            acc = acc - L[:, j, k] * L[:, j, k]
        L[:, j, j] = np.sqrt(acc)
        for i in range(j + 1, N):
            acc = K[:, i, j].copy()
            for k in range(j):
                acc = acc - L[:, i, k] * L[:, j, k]
            L[:, i, j] = acc / L[:, j, j]
    return L


def chol_solve(L, rhs, dtype):
    n, N = L.shape[0], L.shape[1]
    z = np.zeros((n, N), dtype)
    for i in range(N):
        acc = rhs[:, i].copy()
        for k in range(i):
            acc = acc - L[:, i, k] * z[:, k]
        z[:, i] = acc / L[:, i, i]
    y = np.zeros((n, N), dtype)
    for i in range(N - 1, -1, -1):
        acc = z[:, i].copy()
        for k in range(i + 1, N):
            acc = acc - L[:, k, i] * y[:, k]
        y[:, i] = acc / L[:, i, i]
    return y


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _ratio(v, dv, on, dtype):
    """min over the rows `on` with dv < 0 of v / -dv; +inf where there is none.  v, dv [n, 4, 6], on [n, 4]."""
    neg = (dv < 0) & on[:, :, None]
    r = np.where(neg, v / np.where(neg, -dv, dtype(1)), dtype(np.inf))
    return r.reshape(len(v), -1).min(axis=1)


class _Row:
    """The data of the limited rows, [n, ...] in dtype: what the iteration reads."""

    def __init__(self, d, w, stance, rho_s, c, B, f, mu, h, dtype):
        self.d, self.w, self.stance, self.rho, self.c, self.B, self.f, self.mu, self.h, self.dtype = d, w, stance, rho_s, c, B, f, mu, h, dtype
        self.m = (6 * stance.sum(axis=1)).astype(dtype)

    def wrench(self, x):
        r = self.rho.copy()
        for e in range(NEE):
            xe = np.where(self.stance[:, e][:, None], x[:, e], self.dtype(0))
            r[:, 0:3] = r[:, 0:3] - _cross(self.d[:, e], xe)
            r[:, 3:6] = r[:, 3:6] - xe
        return r

    def grad(self, x):
        r = self.wrench(x)
        g = np.zeros_like(x)
        for e in range(NEE):
            ge = (self.c / self.w[:, e])[:, None] * x[:, e] - (_cross(r[:, 0:3], self.d[:, e]) + r[:, 3:6])
            g[:, e] = np.where(self.stance[:, e][:, None], ge, self.dtype(0))
        return g

    def G(self, v):
        return np.stack([g_mul(self.B[:, e], self.mu, v[:, e]) for e in range(NEE)], axis=1)

    def GT(self, y):
        out = np.stack([gt_mul(self.B[:, e], self.mu, y[:, e]) for e in range(NEE)], axis=1)
        return np.where(self.stance[:, :, None], out, self.dtype(0))

    def ssum(self, v):
        """The sum of v [n, 4, 6] over the stance feet, foot after foot, row after row."""
        acc = np.zeros(len(v), self.dtype)
        for e in range(NEE):
            for r in range(6):
                acc = acc + np.where(self.stance[:, e], v[:, e, r], self.dtype(0))
        return acc

    def kkt(self, H, D):
        K = H.copy()
        mu, B = self.mu, self.B
        for e in range(NEE):
            De = D[:, e]
            S = ((De[:, 2] + De[:, 3]) + De[:, 4]) + De[:, 5]
            cnn = (De[:, 0] + De[:, 1]) + (mu * mu) * S
            cn1, cn2, c11, c22 = mu * (De[:, 3] - De[:, 2]), mu * (De[:, 5] - De[:, 4]), De[:, 2] + De[:, 3], De[:, 4] + De[:, 5]
            bn, b1, b2 = B[:, e, 0], B[:, e, 1], B[:, e, 2]
            Tn = (cnn[:, None] * bn + cn1[:, None] * b1) + cn2[:, None] * b2
            T1 = cn1[:, None] * bn + c11[:, None] * b1
            T2 = cn2[:, None] * bn + c22[:, None] * b2
            on = self.stance[:, e]
            for i in range(3):
                for j in range(i + 1):
                    blk = (bn[:, i] * Tn[:, j] + b1[:, i] * T1[:, j]) + b2[:, i] * T2[:, j]
                    K[:, 3 * e + i, 3 * e + j] = np.where(on, H[:, 3 * e + i, 3 * e + j] + blk, H[:, 3 * e + i, 3 * e + j])
        return K


def solve_rows(d, w, stance, rho_s, c, slopes, f, x_fit, mu, f_max, mu_end, max_iter, dtype, ctol=CTOL, rtol=RTOL):
    """The limited path for n rows that all have a stance foot: d, f, x_fit [n, 4, 3], w, stance [n, 4], rho_s [n, 6], c [n], slopes
    [n, 4, 2].  Returns dict(x [n, 4, 3], s, z [n, 4, 6], steps, comp, rd, cap)."""
    n = len(d)
    mu, f_max, mu_end = dtype(np.float64(mu)), dtype(np.float64(f_max)), dtype(np.float64(mu_end))
    one, zero, inf = dtype(1), dtype(0), dtype(np.inf)
    B = np.stack([basis(slopes[:, e, 0], slopes[:, e, 1], dtype) for e in range(NEE)], axis=1)
    h = np.zeros((n, NEE, 6), dtype)
    h[:, :, 1] = f_max
    R = _Row(d, w, stance, rho_s, c, B, f, mu, h, dtype)
    st3 = stance[:, :, None]
    # start
    gam_lo, gam_hi = np.minimum(one, f_max / dtype(4)), f_max / dtype(2)
    x_int = np.zeros((n, NEE, 3), dtype)
    for e in range(NEE):
        gam = np.minimum(np.maximum(_dot(B[:, e, 0], f[:, e]), gam_lo), gam_hi)
        x_int[:, e] = B[:, e, 0] * gam[:, None] - f[:, e]
    x_int = np.where(st3, x_int, zero)
    s_int = h - R.G(f + x_int)
    dirn = np.where(st3, x_fit - x_int, zero)
    theta = np.minimum(one, dtype(np.float64(0.9)) * _ratio(s_int, -R.G(dirn), stance, dtype))
    x = x_int + theta[:, None, None] * dirn
    s = h - R.G(f + x)
    s = np.where(st3, s, one)
    z = one / s
    H = hessian(d, w, stance, c, dtype)
    q = R.grad(np.zeros_like(x))
    qinf = np.abs(q).reshape(n, -1).max(axis=1)
    steps, done, cap = np.zeros(n, np.int32), np.zeros(n, bool), np.zeros(n, bool)
    comp, rdn = np.zeros(n, dtype), np.zeros(n, dtype)
    p99, ten = dtype(np.float64(0.99)), dtype(10)
    for it in range(int(max_iter) + 1):
        sz = s * z
        muk = R.ssum(sz) / R.m
        grad = R.grad(x)
        rd = grad + R.GT(z)
        comp_now = np.where(st3, np.abs(sz - mu_end), zero).reshape(n, -1).max(axis=1) / mu_end
        rd_now = np.abs(rd).reshape(n, -1).max(axis=1)
        comp, rdn = np.where(done, comp, comp_now), np.where(done, rdn, rd_now)
        conv = (comp_now <= dtype(np.float64(ctol))) & (rd_now <= dtype(np.float64(rtol)) * (one + qinf))
        done = done | conv
        if it == int(max_iter):
            cap = ~done
            break
        if done.all():
            break
        D = z / s
        L = cholesky(R.kkt(H, D), dtype)
        pred = muk > ten * mu_end
        dxa = chol_solve(L, (-grad).reshape(n, 12), dtype).reshape(n, NEE, 3)
        dsa = -R.G(dxa)
        dza = -z - D * dsa
        ala = np.minimum(one, np.minimum(_ratio(s, dsa, stance, dtype), _ratio(z, dza, stance, dtype)))
        mua = R.ssum((s + ala[:, None, None] * dsa) * (z + ala[:, None, None] * dza)) / R.m
        ratio = mua / muk
        target = np.where(pred, np.maximum(((ratio * ratio) * ratio) * muk, mu_end), mu_end)
        rc = target[:, None, None] - sz
        rc = np.where(pred[:, None, None], rc - dsa * dza, rc)
        rhs = -(rd + R.GT(rc / s))
        dx = chol_solve(L, rhs.reshape(n, 12), dtype).reshape(n, NEE, 3)
        ds = -R.G(dx)
        dz = rc / s - D * ds
        al = np.minimum(one, p99 * np.minimum(_ratio(s, ds, stance, dtype), _ratio(z, dz, stance, dtype)))
        go = ~done
        al = np.where(go, al, zero)[:, None, None]
        x = np.where(st3, x + al * dx, x)
        s = np.where(st3, s + al * ds, s)
        z = np.where(st3, z + al * dz, z)
        steps = steps + go.astype(np.int32)
    return dict(x=x, s=s, z=z, steps=steps, comp=comp, rd=rdn, cap=cap, B=B, H=H, q=q, h=h)


def objective_gap(d, w, stance, rho_s, c, x_fit, x, dtype):
    """objective(x) - objective(x_fit), formed as grad_fit . D + 1/2 (|A~ D|^2 + c sum |D_e|^2 / w_e), D = x - x_fit."""
    n = len(d)
    R = _Row(d, w, stance, rho_s, c, None, None, None, None, dtype)
    g = R.grad(x_fit)
    Dl = np.where(stance[:, :, None], x - x_fit, dtype(0))
    AD = np.zeros((n, 6), dtype)
    lin, quad = np.zeros(n, dtype), np.zeros(n, dtype)
    for e in range(NEE):
        AD[:, 0:3] = AD[:, 0:3] + _cross(d[:, e], Dl[:, e])
        AD[:, 3:6] = AD[:, 3:6] + Dl[:, e]
        lin = lin + _dot(g[:, e], Dl[:, e])
        quad = quad + np.where(stance[:, e], (c / w[:, e]) * _dot(Dl[:, e], Dl[:, e]), dtype(0))
    sq = ((((AD[:, 0] * AD[:, 0] + AD[:, 1] * AD[:, 1]) + AD[:, 2] * AD[:, 2]) + AD[:, 3] * AD[:, 3]) + AD[:, 4] * AD[:, 4]) + AD[:, 5] * AD[:, 5]
    return lin + dtype(np.float64(0.5)) * (sq + quad)


def qp_rows(L, nodes, t0, hz, first_row, n_rows, params, qp=None, terrain=None, mass_scale=1.0, joint=None, times=None,
            dtype=np.float64, detail=False, ctol=CTOL, rtol=RTOL):
    """The rows first_row .. first_row + n_rows - 1 of the plan `nodes`: (rows [n, 32] in dtype, qrows [n, 8] in dtype, status [n]
    int32; the module's docstring has the columns and the bits).  The arguments are force_fit.fit_rows'; qp: a QpParams (None:
    qp_params(params)).  detail: also a dict -- fit's detail, fit_rows (the fit's table), limited [n], fit_value [n] the largest
    limit-row value G f_fit - h over the stance feet (-inf without stance), slack, z [n, 4, 6] (NaN where not solved), x [n, 4, 3]."""
    qp = qp_params(params) if qp is None else qp
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        return _qp_rows(L, nodes, t0, hz, first_row, n_rows, params, qp, terrain, mass_scale, joint, times, dtype, detail, ctol, rtol)


def _qp_rows(L, nodes, t0, hz, first_row, n_rows, params, qp, terrain, mass_scale, joint, times, dtype, detail, ctol, rtol):
    fit_out, fit_status, D = ff.fit_rows(L, nodes, t0, hz, first_row, n_rows, params, qp, terrain, mass_scale, joint, times, dtype, True)
    n = len(fit_out)
    stance, d, w, f, df = D["stance"], D["d"], D["w"], D["f"], D["df"]
    cnt = stance.sum(axis=1)
    bad = (fit_status & NONFINITE) != 0
    mu, f_max = dtype(np.float64(qp.mu)), dtype(np.float64(qp.f_max))
    arm = dtype(np.float64(qp.arm))
    rho_s = np.concatenate([D["rho"][:, 0:3] / arm, D["rho"][:, 3:6]], axis=1)
    c = dtype(np.float64(qp.damping)) * cnt.astype(dtype)
    h = np.zeros((n, NEE, 6), dtype)
    h[:, :, 1] = f_max
    Bs = np.stack([basis(D["slopes"][:, e, 0], D["slopes"][:, e, 1], dtype) for e in range(NEE)], axis=1)
    f_fit = fit_out[:, 1:13].reshape(n, NEE, 3)
    val = np.stack([g_mul(Bs[:, e], mu, f_fit[:, e]) for e in range(NEE)], axis=1) - h
    inside = (np.where(stance[:, :, None], val, dtype(-1)) <= 0).reshape(-1, 24).all(axis=1)
    limited = (cnt > 0) & ~bad & ~inside
    fit_value = np.where(stance[:, :, None], val, dtype(-np.inf)).reshape(-1, 24).max(axis=1)
    out, status = fit_out.copy(), (fit_status & 7).astype(np.int32)
    qrows = np.zeros((n, QP_COLS), dtype)
    slack = np.where(stance[:, :, None], -val, dtype(np.nan))
    zs = np.full((n, NEE, 6), np.nan, dtype)
    x = np.where(stance[:, :, None], df, dtype(0))
    idx = np.nonzero(limited)[0]
    if len(idx):
        S = solve_rows(d[idx], w[idx], stance[idx], rho_s[idx], c[idx], D["slopes"][idx], f[idx], x[idx], qp.mu, qp.f_max, qp.mu_end,
                       qp.max_iter, dtype, ctol, rtol)
        xs = S["x"]
        res_ang, res_lin, sq = D["rho"][idx, 0:3].copy(), D["rho"][idx, 3:6].copy(), np.zeros(len(idx), dtype)
        p = D["p"][idx]
        dsq = np.zeros(len(idx), dtype)
        for e in range(NEE):
            on = stance[idx, e]
            de = np.where(on[:, None], xs[:, e], dtype(0))
            res_ang = res_ang - _cross(p[:, e], de)
            res_lin = res_lin - de
            sq = sq + ((de[:, 0] * de[:, 0] + de[:, 1] * de[:, 1]) + de[:, 2] * de[:, 2])
            dd = np.where(on[:, None], xs[:, e] - x[idx, e], dtype(0))
            dsq = dsq + ((dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2])
        change = np.sqrt(sq)
        gap = objective_gap(d[idx], w[idx], stance[idx], rho_s[idx], c[idx], x[idx], xs, dtype)
        nf = ~(np.isfinite(res_ang).all(axis=1) & np.isfinite(res_lin).all(axis=1) & np.isfinite(change) & np.isfinite(xs).all(axis=(1, 2)))
        fq = np.where(stance[idx][:, :, None] & ~nf[:, None, None], f[idx] + xs, f[idx])
        nan = np.where(nf, dtype(np.nan), dtype(0))
        out[idx, 1:13] = fq.reshape(len(idx), 12)
        out[idx, 13:16], out[idx, 16:19], out[idx, 19] = res_ang + nan[:, None], res_lin + nan[:, None], change + nan
        st_on = stance[idx][:, :, None]
        smin = np.where(st_on, S["s"], dtype(np.inf)).reshape(-1, 24).min(axis=1)
        zmax = np.where(st_on, S["z"], dtype(0)).reshape(-1, 24).max(axis=1)
        qrows[idx, 0] = S["steps"].astype(dtype)
        qrows[idx, 1], qrows[idx, 2], qrows[idx, 3], qrows[idx, 4] = S["comp"] + nan, S["rd"] + nan, smin + nan, zmax + nan
        qrows[idx, 5], qrows[idx, 6] = np.sqrt(dsq) + nan, gap + nan
        slack[idx] = np.where(st_on, S["s"], dtype(np.nan))
        zs[idx] = np.where(st_on, S["z"], dtype(np.nan))
        x[idx] = xs
        status[idx] |= LIMITED | np.where(S["cap"], CAP, 0).astype(np.int32) | np.where(nf, NONFINITE, 0).astype(np.int32)
        if joint is not None:
            qj = np.asarray(joint, np.float64).reshape(n, joints.JOINT_COLS)[idx, 1:13]
            for e in range(NEE):
                out[idx, 20 + 3 * e:23 + 3 * e] = joints.feed_forward(e, qj[:, 3 * e:3 * e + 3], D["th"][idx], fq[:, e], qp, dtype)
    # the slacks' columns and bits, both paths (a non-finite row: nothing)
    act = stance[:, :, None] & (slack <= dtype(np.float64(qp.act_tol))) & ~((status & NONFINITE) != 0)[:, None, None]
    fitp = (cnt > 0) & ~limited & ~bad
    qrows[fitp, 3] = np.where(stance[fitp][:, :, None], slack[fitp], dtype(np.inf)).reshape(-1, 24).min(axis=1)
    qrows[:, 7] = act.reshape(-1, 24).sum(axis=1).astype(dtype)
    for e in range(NEE):
        status |= np.where(act[:, e].any(axis=1), ACTIVE << e, 0).astype(np.int32)
    qrows[bad, 1:7] = dtype(np.nan)
    if detail:
        D = dict(D, fit_rows=fit_out, fit_status=fit_status, limited=limited, fit_value=fit_value, slack=slack, z=zs, x=x, B=Bs, rho_s=rho_s, c=c)
        return out, qrows, status, D
    return out, qrows, status


def violations(table, qtable):
    """[n, 4] float64: the violation of every family per row; a non-finite column counts as +inf."""
    T = np.asarray(table, np.float64).reshape(-1, COLS)
    Q = np.asarray(qtable, np.float64).reshape(-1, QP_COLS)
    inf = np.float64(np.inf)
    fin = np.isfinite(T)
    v = np.zeros((len(T), 4))
    v[:, 0] = np.where(fin[:, 13:16], np.abs(T[:, 13:16]), inf).max(axis=1, initial=0.0)
    v[:, 1] = np.where(fin[:, 16:19], np.abs(T[:, 16:19]), inf).max(axis=1, initial=0.0)
    v[:, 2] = np.where(fin[:, 19], np.abs(T[:, 19]), inf)
    v[:, 3] = np.where(np.isfinite(Q[:, 5]), np.abs(Q[:, 5]), inf)
    return v


def empty_summary(*shape):
    return ff.empty_summary(*shape)


def summarise(table, qtable, first_row, tol):
    """The four families of a float64 table [n, 32] and its solve table [n, 8] as four SUMMARY records (plan_check.summarise's
    semantics: the largest violation, the lowest row that attains it counted from first_row, the rows over tol[f])."""
    v = violations(table, qtable)
    out = empty_summary()
    tol = np.asarray(tol, np.float64).reshape(4)
    if len(v):
        out["max"] = v.max(axis=0)
        out["row"] = np.int64(first_row) + np.argmax(v == out["max"][None, :], axis=0)
        out["count"] = (v > tol[None, :]).sum(axis=0)
    return out


accumulate = pc.accumulate


def report_lines(summary, t0=0.0, hz=1000.0, tol=None):
    """One line per family of four SUMMARY records, in plan_check.report_lines' format."""
    lines = []
    for i, name in enumerate(FAMILIES):
        s = summary[i]
        when = "-" if s["row"] < 0 else "%.3f s (row %d)" % (float(t0) + int(s["row"]) / float(hz), int(s["row"]))
        over = "" if tol is None else " over %.1e" % float(tol[i])
        lines.append("force qp   %-8s max %.3e %-3s at %s, %d rows%s" % (name, float(s["max"]), UNITS[i], when, int(s["count"]), over))
    return lines
