"""numpy statement of the terrain look-up (TEST INFRASTRUCTURE, like everything under oracle/).

Every kernel that meets a heightfield goes through terrain_at of csrc/kernels.hpp; the C oracle, plan_check.terrain_at and
heightfield.height_at restate it with the same floor / clamp / ix + 1 logic.  This file states the rule once more WITHOUT a
cell index, so that a wrong choice in that logic is not shared:

  * grid coordinates  fx = (x - x0) / cell,  p = clip(fx, 0, nx - 1);  fy, q likewise
  * bilinear height   h = sum_i sum_j H[i, j] L(p - i) L(q - j)  over ALL nodes, L(t) = max(0, 1 - |t|) the hat function
  * slopes            from the hat's right-hand derivative L'+ (+1 on [-1, 0), -1 on [0, 1), 0 elsewhere):
                      hx = sum sum H L'+(p - i) L(q - j) / cell, and 0 where fx <= 0 or fx >= nx - 1 (the point is clamped);
                      hy likewise;  hxy = sum sum H L'+ L'+ / cell^2, and 0 where either axis is clamped
  * nearest cell      the node that minimises |p - i|, a tie going to the larger index; likewise in y; all slopes 0
  * a non-finite coordinate has no terrain: NaN in all four outputs

and the five force rows of a foothold with their derivatives with respect to the foothold's x and y, from the definition of
the terrain's normal and tangents.  dtype = np.longdouble is the reference, dtype = np.float64 the same formulas in the
kernels' precision: the distance between the two is the rounding floor the tests derive their gates from.  It imports
nothing from the product package and nothing from the C oracle."""
import numpy as np


def _hat(t, dtype):
    return np.maximum(dtype(0), dtype(1) - np.abs(t))


def _hat_right(t, dtype):
    """Right-hand derivative of the hat function."""
    return np.where((t >= -1) & (t < 0), dtype(1), np.where((t >= 0) & (t < 1), dtype(-1), dtype(0)))


def grid_coordinate(x, origin, cell, dtype=np.longdouble):
    """fx = (x - origin) / cell in dtype, of float64 inputs."""
    return (np.asarray(x, np.float64).astype(dtype) - dtype(np.float64(origin))) / dtype(np.float64(cell))


def lookup(H, cell, x0, y0, x, y, mode, dtype=np.longdouble):
    """(h, hx, hy, hxy) [n] in dtype of the grid H [nx, ny] (node (i, j) at x0 + i cell, y0 + j cell) under the points x, y [n]:
    mode 0 bilinear with zero slope where the point is clamped to the border, mode 1 the nearest cell."""
    H = np.asarray(H, np.float64)
    if H.ndim != 2 or H.size == 0:
        raise ValueError("H is a grid [nx, ny]")
    nx, ny = H.shape
    Hd = H.astype(dtype)
    x, y = np.atleast_1d(np.asarray(x, np.float64)), np.atleast_1d(np.asarray(y, np.float64))
    fx, fy = grid_coordinate(x, x0, cell, dtype), grid_coordinate(y, y0, cell, dtype)
    bad = ~(np.isfinite(fx) & np.isfinite(fy))
    fx, fy = np.where(bad, dtype(0), fx), np.where(bad, dtype(0), fy)
    nan = np.where(bad, dtype(np.nan), dtype(0))
    p, q = np.clip(fx, dtype(0), dtype(nx - 1)), np.clip(fy, dtype(0), dtype(ny - 1))
    tp = p[:, None] - np.arange(nx).astype(dtype)[None, :]                  # p - i for every node of the axis
    tq = q[:, None] - np.arange(ny).astype(dtype)[None, :]
    zero = np.zeros(len(x), dtype)
    if mode == 1:
        # the last of the nodes at the smallest distance
        ix = nx - 1 - np.argmin(np.abs(tp)[:, ::-1], axis=1)
        iy = ny - 1 - np.argmin(np.abs(tq)[:, ::-1], axis=1)
        return Hd[ix, iy] + nan, zero + nan, zero + nan, zero + nan
    if mode != 0:
        raise ValueError("mode is 0 (bilinear) or 1 (nearest cell)")
    Lx, Ly, Dx, Dy = _hat(tp, dtype), _hat(tq, dtype), _hat_right(tp, dtype), _hat_right(tq, dtype)
    c = dtype(np.float64(cell))
    cx, cy = (fx <= 0) | (fx >= nx - 1), (fy <= 0) | (fy >= ny - 1)

    def tensor(A, B):
        return ((A @ Hd) * B).sum(axis=1)
    h = tensor(Lx, Ly)
    hx = np.where(cx, dtype(0), tensor(Dx, Ly) / c)
    hy = np.where(cy, dtype(0), tensor(Lx, Dy) / c)
    hxy = np.where(cx | cy, dtype(0), tensor(Dx, Dy) / (c * c))
    return h + nan, hx + nan, hy + nan, hxy + nan


def _unit(v, vx, vy):
    """A vector field v [n, 3] with its x and y derivatives, normalised: b = v / |v| and b' = (v' - b (b . v')) / |v|."""
    nn = np.sqrt((v * v).sum(axis=1))[:, None]
    b = v / nn
    return b, (vx - b * (b * vx).sum(axis=1)[:, None]) / nn, (vy - b * (b * vy).sum(axis=1)[:, None]) / nn


def force_rows(f, hx, hy, hxy, mu, dtype=np.longdouble):
    """(values, d_dx, d_dy), each [n, 5] in dtype: the five force rows n . f, (t1 - mu n) . f, (t1 + mu n) . f, (t2 - mu n) . f,
    (t2 + mu n) . f of the forces f [n, 3] at footholds where the terrain has the slopes hx, hy and the mixed derivative hxy
    [n], and the rows' derivatives with respect to the foothold's x and y.  n = (-hx, -hy, 1), t1 = (1, 0, hx),
    t2 = (0, 1, hy), each normalised; inside a cell d hx / dx = d hy / dy = 0 and d hx / dy = d hy / dx = hxy."""
    f = np.asarray(f, np.float64).reshape(-1, 3).astype(dtype)
    hx, hy, hxy = (np.asarray(a).astype(dtype).reshape(-1) for a in (hx, hy, hxy))
    one, zero = np.ones(len(f), dtype), np.zeros(len(f), dtype)

    def field(*cols):
        return np.stack(cols, axis=1)
    n = _unit(field(-hx, -hy, one), field(zero, -hxy, zero), field(-hxy, zero, zero))
    t1 = _unit(field(one, zero, hx), field(zero, zero, zero), field(zero, zero, hxy))
    t2 = _unit(field(zero, one, hy), field(zero, zero, hxy), field(zero, zero, zero))
    mu = dtype(np.float64(mu))
    out = []
    for k in range(3):                                                   # value, d / dx, d / dy
        vecs = (n[k], t1[k] - mu * n[k], t1[k] + mu * n[k], t2[k] - mu * n[k], t2[k] + mu * n[k])
        out.append(np.stack([(v * f).sum(axis=1) for v in vecs], axis=1))
    return tuple(out)
