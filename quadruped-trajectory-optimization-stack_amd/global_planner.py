"""Global planner: A* over the boolean map + cubic "spine" + start/goal pair generation.
Counterpart of QTOS/planner.py (``PATH_Solver`` :282-457, ``Global_Planner`` :15-280), pure
numpy/scipy like the reference (not a GPU workload); it produces the batch axis of the local
planner (start / goal per re-plan).  Quirks kept on purpose: the spline's end point is appended
WITHOUT the origin shift (:410,412), pairs are popped LIFO (QTOS/containers.py:171-181).
"""
import heapq
import math

import numpy as np
from scipy.interpolate import CubicSpline


class PathSolver:
    def __init__(self, map_yx, start, goal, step_size=1.0, grid_res=0.1, origin_x_shift=1.0,
                 origin_y_shift=1.0, bool_map=None):
        self.visual_map = np.asarray(map_yx)
        self.bool_map = self.visual_map if bool_map is None else np.asarray(bool_map)
        self.grid_res, self.step_size = grid_res, step_size
        self.origin_x_shift, self.origin_y_shift = origin_x_shift, origin_y_shift
        self.solution_flag = False
        self.robot_goal = list(goal)
        self.start_idx = self.convert_2_idx(start[0], start[1])
        self.goal_idx = self.convert_2_idx(goal[0], goal[1])
        self.path = self.astar(self.start_idx, self.goal_idx)
        self.predicted_t = np.linalg.norm(np.array(start[0:2]) - np.array(goal[0:2])) / step_size * 10
        if self.solution_flag:
            self._solve()

    def convert_2_idx(self, x, y):
        return (math.floor((y + self.origin_y_shift) / self.grid_res),
                math.floor((x + self.origin_x_shift) / self.grid_res))

    @staticmethod
    def heuristic(a, b):
        return np.sqrt((b[0] - a[0]) ** 2 + (b[1] - a[1]) ** 2)

    def astar(self, start, goal, height_bound=0.2):
        """4-neighbour A*, Euclidean cost, cells with bool_map > height_bound are blocked
        (QTOS/planner.py:354-399; same tie-breaking: heap of (f, cell))."""
        neighbors = [(0, 1), (0, -1), (1, 0), (-1, 0)]
        close_set, came_from = set(), {}
        gscore = {start: 0}
        oheap = [(self.heuristic(start, goal), start)]
        while oheap:
            current = heapq.heappop(oheap)[1]
            if current == goal:
                data = []
                while current in came_from:
                    data.append(current)
                    current = came_from[current]
                self.solution_flag = True
                return [start] + data[::-1]
            close_set.add(current)
            for i, j in neighbors:
                nb = (current[0] + i, current[1] + j)
                g = gscore[current] + self.heuristic(current, nb)
                if not (0 <= nb[0] < self.bool_map.shape[0] and 0 <= nb[1] < self.bool_map.shape[1]):
                    continue
                if self.bool_map[nb[0]][nb[1]] > height_bound:
                    continue
                if nb in close_set and g >= gscore.get(nb, 0):
                    continue
                if g < gscore.get(nb, 0) or nb not in [e[1] for e in oheap]:
                    came_from[nb] = current
                    gscore[nb] = g
                    heapq.heappush(oheap, (g + self.heuristic(nb, goal), nb))
        return None

    def _solve(self):
        sub = self.path[::2]
        t = np.linspace(0, self.predicted_t, len(sub) + 1)
        xs = [(c[1] * self.grid_res) - self.origin_x_shift for c in sub]
        xs.append(self.path[-1][1] * self.grid_res)          # sic: no origin shift on the end point
        ys = [(c[0] * self.grid_res) - self.origin_y_shift for c in sub]
        ys.append(self.path[-1][0] * self.grid_res)
        self.spine_x_track = CubicSpline(t, xs)
        self.spine_y_track = CubicSpline(t, ys)


class GlobalPlanner:
    def __init__(self, map_yx, start, robot_goal, step_size=1.0, resolution=0.1, lookahead=7500,
                 hz=1000, bool_map=None, history=500):
        self.map = np.asarray(map_yx)
        self.grid_res, self.step_size = resolution, step_size
        self.lookahead, self.hz = lookahead, hz
        self.approx_z = 0.24
        self.origin_x_shift = self.origin_y_shift = 1.0
        self.robot_goal = list(robot_goal)
        self.path_solver = PathSolver(self.map, start, robot_goal, step_size, resolution, bool_map=bool_map)
        self.max_t = self.path_solver.predicted_t
        self._stack, self._cap = [], history

    def convert_2_idx(self, x, y):
        return (math.floor((y + self.origin_y_shift) / self.grid_res),
                math.floor((x + self.origin_x_shift) / self.grid_res))

    def get_map_height(self, pos):
        try:
            row, col = self.convert_2_idx(pos[0], pos[1])
            return self.map[row, col]
        except Exception:
            r, c = self.map.shape
            return self.map[r - 1, c // 2]

    def spine_step(self, com, timestep, total_traj_time=5.0, tol=0.00001):
        tf = timestep + total_traj_time
        sx, sy = self.path_solver.spine_x_track, self.path_solver.spine_y_track
        xf = sx(tf).item() if np.abs(sx(tf)) > tol else 0.0
        yf = sy(tf).item() if np.abs(sy(tf)) > tol else 0.0
        goal = np.array([xf, yf, self.get_map_height((xf, yf)) + self.approx_z])
        return com + np.clip(goal - com, -self.step_size, self.step_size)

    def lookahead_timestamp(self, time):
        return time + round(self.lookahead / self.hz, 3)

    def update(self, timestep):
        """Push one (start, goal) pair for a re-plan issued at ``timestep`` (QTOS/planner.py:195-230)."""
        lt = self.lookahead_timestamp(timestep)
        start = np.array([self.path_solver.spine_x_track(lt), self.path_solver.spine_y_track(lt), 0.0])
        start[2] = self.get_map_height(start[0:2]) + self.approx_z
        goal = self.spine_step(start, lt)
        if len(self._stack) >= self._cap:
            self._stack.pop(0)
        self._stack.append((start, goal))

    def pop(self):
        return self._stack.pop()   # LIFO, like Limited_Stack

    def empty(self):
        return not self._stack


# ---- the goals of B receding windows from their global paths: the rule of k_path_goal (qtos_path_goal*) in numpy ----------
# What Global_Planner.update / spine_step and Combiner.plan_init / spine_step do for one robot through scipy objects, on plain
# arrays for B windows at once.  Every operation below is one rounded IEEE double operation, in the order the kernel performs
# them: the kernel equals these lines to the bit (a NaN equals a NaN; IEEE leaves its payload open).

PATH_BASES = {"spine": 0, "state": 1}


def path_table(planners):
    """The spines of a list of ``GlobalPlanner`` (or ``PathSolver``) as plain arrays, a dict of
    knots [n_paths, max_pieces + 1]       scipy's ``CubicSpline.x``; rows of shorter paths repeat their last knot
    coef [n_paths, 2, 4, max_pieces]      ``spine_x_track.c`` and ``spine_y_track.c`` (c[k, i] multiplies (t - x[i]) ** (3 - k)); padding 0
    n_pieces [n_paths] (int32, >= 1)      robot_goal [n_paths, 3] (NaN where a planner has none: ``clamp_x`` then never clips)"""
    solvers = [getattr(p, "path_solver", p) for p in planners]
    if not solvers:
        raise ValueError("path_table needs at least one path")
    n = [len(s.spine_x_track.x) - 1 for s in solvers]
    mp = max(n)
    knots = np.zeros((len(solvers), mp + 1))
    coef = np.zeros((len(solvers), 2, 4, mp))
    goal = np.full((len(solvers), 3), np.nan)
    for j, (p, s) in enumerate(zip(planners, solvers)):
        x = np.asarray(s.spine_x_track.x, np.float64)
        if n[j] < 1 or not np.array_equal(x, np.asarray(s.spine_y_track.x, np.float64)):
            raise ValueError("path %d: the x and y spines need the same knots, two at least" % j)
        knots[j, :n[j] + 1] = x
        knots[j, n[j] + 1:] = x[-1]
        coef[j, 0, :, :n[j]] = s.spine_x_track.c
        coef[j, 1, :, :n[j]] = s.spine_y_track.c
        g = [float(v) for v in (getattr(p, "robot_goal", None) or getattr(s, "robot_goal", None) or [])][:3]
        goal[j, :len(g)] = g
    return dict(knots=knots, coef=coef, n_pieces=np.asarray(n, np.int32), robot_goal=goal)


def spine_eval(knots_row, coef_row, n, t):
    """One spine at time t (a scalar), as ``CubicSpline.__call__`` gives it, to the bit: knots_row [>= n + 1], coef_row
    [4, >= n] of ``path_table``, n pieces.  The piece is i = clip(searchsorted(x[:n + 1], t, 'right') - 1, 0, n - 1) -- times
    before the first knot use piece 0, times at or beyond the last knot piece n - 1, as scipy extrapolates -- and the value is
    summed in scipy's order, which is not Horner's: res = 0; z = 1; four times res = res + c[3 - kp, i] * z; z = z * s."""
    x = np.asarray(knots_row, np.float64)
    c = np.asarray(coef_row, np.float64)
    n = int(n)
    t = np.float64(t)
    i = min(max(int(np.searchsorted(x[:n + 1], t, side="right")) - 1, 0), n - 1)
    s = t - x[i]
    res, z = np.float64(0.0), np.float64(1.0)
    for kp in range(4):
        res = res + c[3 - kp, i] * z
        z = z * s
    return res


def _spine_eval_rows(knots, coef, n, t):
    """``spine_eval`` for B rows at once: knots [B, mp + 1], coef [B, 4, mp], n [B], t [B]."""
    B = len(t)
    # (a row's padding repeats its last knot: it is counted only for t at or beyond the end, where the clip decides)
    i = np.where(np.isnan(t), n - 1, np.clip((knots <= t[:, None]).sum(axis=1) - 1, 0, n - 1))
    rows = np.arange(B)
    s = t - knots[rows, i]
    res, z = np.zeros(B), np.ones(B)
    for kp in range(4):
        res = res + coef[rows, 3 - kp, i] * z
        z = z * s
    return res


def map_height(map_yx, x, y, cell, ox, oy):
    """``GlobalPlanner.get_map_height`` on arrays: row = floor((y + oy) / cell), col = floor((x + ox) / cell); a negative
    index down to -rows / -cols wraps as Python's does; anything else (out of range, non-finite) gives map[rows - 1, cols // 2].
    map_yx is [rows, cols], or [B, rows, cols] with one grid per point."""
    m = np.asarray(map_yx, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rows, cols = m.shape[-2:]
    with np.errstate(invalid="ignore", over="ignore"):
        fr, fc = np.floor((y + oy) / cell), np.floor((x + ox) / cell)
        ok = (fr >= -rows) & (fr < rows) & (fc >= -cols) & (fc < cols)       # (tested in double: nothing huge or NaN becomes an int)
    r = np.where(ok, fr, rows - 1).astype(np.int64)
    c = np.where(ok, fc, cols // 2).astype(np.int64)
    r, c = np.where(r < 0, r + rows, r), np.where(c < 0, c + cols, c)
    return m[r, c] if m.ndim == 2 else m[np.arange(m.shape[0]), r, c]


def _path_param(params, name):
    v = params[name] if isinstance(params, dict) else getattr(params, name)
    return PATH_BASES[v] if name == "base" and isinstance(v, str) else v


def path_goal(table, path_id, map_yx, map_id, clock, offset, start, params, done=None):
    """The goals of B windows' next plans from their global paths: the rule of k_path_goal.  table: ``path_table``; path_id [B]
    (None: window b follows path b); map_yx [n_maps, rows, cols] (None: every height 0) with map_id [B] (None: map 0); clock [B]
    the plan time of row 0 of the plans being executed; offset [B] the hand-over's (None: 0); start [B, >= 3] the state the new
    plans start from (None where nothing reads it); done [B] the windows' done bits so far (None: 0).  params: a
    ``capi.QtosPathGoal`` or a dict of its fields (horizon, step_size, tol, z_offset, cell, origin_x, origin_y, t_stop, stop_dist,
    base "spine" | "state" or 0 | 1, clamp_x, advance_clock, hold_done).  Per window b, p = path_id[b]:
      lt = clock + offset, tf = lt + horizon
      sx = X_p(tf), 0.0 unless |sx| > tol; sy likewise; gz = map_height(sx, sy) + z_offset
      clamp_x: sx = min(sx, robot_goal[p][0])                      (Combiner.spine_step: after gz is read)
      base "spine": (X_p(lt), Y_p(lt), map_height(X_p(lt), Y_p(lt)) + z_offset)    (Global_Planner.update);  "state": start[b][0:3]
      goal = base + clip((sx, sy, gz) - base, -step_size, step_size)
      bit 0: t_end[p] < lt - t_stop;  bit 1: stop_dist > 0 and |start[b][0:2] - goal[0:2]| < stop_dist;  done[b] |= bits
      hold_done: goal = start[b][0:3] where done[b] != 0;  advance_clock: clock[b] = lt
    Returns (goal [B, 3], done [B] int32, clock [B]) as new arrays."""
    g = lambda name: _path_param(params, name)
    clock = np.asarray(clock, np.float64).reshape(-1)
    B = len(clock)
    knots_all, coef_all = np.asarray(table["knots"], np.float64), np.asarray(table["coef"], np.float64)
    n_all = np.asarray(table["n_pieces"], np.int64)
    mp = coef_all.shape[3]
    p = np.arange(B) if path_id is None else np.asarray(path_id, np.int64).reshape(B)
    p = np.clip(p, 0, len(n_all) - 1)
    n = np.clip(n_all[p], 1, mp)
    knots, cx, cy = knots_all[p], coef_all[p, 0], coef_all[p, 1]
    grids = None
    if map_yx is not None:
        m = np.asarray(map_yx, np.float64)
        m = m[None] if m.ndim == 2 else m
        mid = np.zeros(B, np.int64) if map_id is None else np.clip(np.asarray(map_id, np.int64).reshape(B), 0, len(m) - 1)
        grids = m[mid]
    cell, ox, oy, zo = float(g("cell")), float(g("origin_x")), float(g("origin_y")), float(g("z_offset"))
    height = (lambda x, y: np.zeros(B)) if grids is None else (lambda x, y: map_height(grids, x, y, cell, ox, oy))
    st = None if start is None else np.asarray(start, np.float64).reshape(B, -1)
    base, step, stop_dist = int(g("base")), float(g("step_size")), float(g("stop_dist"))
    hold = bool(g("hold_done"))
    if st is None and (base == 1 or stop_dist > 0 or hold):
        raise ValueError("start is read by base='state', stop_dist > 0 and hold_done")
    with np.errstate(invalid="ignore", over="ignore"):
        lt = clock + (np.zeros(B) if offset is None else np.asarray(offset, np.float64).reshape(B))
        tf = lt + float(g("horizon"))
        sx, sy = _spine_eval_rows(knots, cx, n, tf), _spine_eval_rows(knots, cy, n, tf)
        sx = np.where(np.abs(sx) > float(g("tol")), sx, 0.0)
        sy = np.where(np.abs(sy) > float(g("tol")), sy, 0.0)
        gz = height(sx, sy) + zo
        if g("clamp_x"):
            rgx = np.asarray(table["robot_goal"], np.float64)[p, 0]
            sx = np.where(sx > rgx, rgx, sx)
        if base == 0:
            bx, by = _spine_eval_rows(knots, cx, n, lt), _spine_eval_rows(knots, cy, n, lt)
            bz = height(bx, by) + zo
        elif base == 1:
            bx, by, bz = st[:, 0], st[:, 1], st[:, 2]
        else:
            raise ValueError("base is 'spine' (0) or 'state' (1)")
        basept = np.stack([bx, by, bz], axis=1)
        goal = basept + np.clip(np.stack([sx, sy, gz], axis=1) - basept, -step, step)
        bits = (knots[np.arange(B), n] < lt - float(g("t_stop"))).astype(np.int32)
        if stop_dist > 0:
            dx, dy = st[:, 0] - goal[:, 0], st[:, 1] - goal[:, 1]
            bits |= 2 * (np.sqrt(dx * dx + dy * dy) < stop_dist).astype(np.int32)
    done_out = bits | (np.zeros(B, np.int32) if done is None else np.asarray(done, np.int32).reshape(B))
    if hold:
        goal = np.where((done_out != 0)[:, None], st[:, 0:3], goal)
    return goal, done_out.astype(np.int32), (lt if g("advance_clock") else clock.copy())


# ---- the global paths of B receding windows: the rule of k_path_plan (qtos_path_plan*) in numpy ---------------------------
# What PATH_Solver does for one robot -- A* over the boolean map, every second cell a point of two not-a-knot cubics -- on plain
# arrays, in a fixed order of IEEE double operations: the kernel equals these lines to the bit.  ``path_cells`` is
# ``PathSolver.astar`` cell for cell, ``spine_fit`` is scipy's ``CubicSpline(t, y).c`` up to the rounding of another
# elimination order, ``path_plan`` puts them together into the table ``path_goal`` reads.

PATH_NEIGHBOURS = ((0, 1), (0, -1), (1, 0), (-1, 0))      # (d row, d col), the order PathSolver.astar visits them in
PATH_STATUS = {0: "found", 1: "no path", 2: "more than max_cells cells", 3: "open list or pop cap", 4: "T is not > 0"}
PATH_MAX_GRID, PATH_MAX_OPEN = 16384, 4096                # what the kernel's LDS is laid out for
PATH_DONE_BIT = 4                                         # bit 2 of a window's done bits: it has no path


def _cell_of(v, o, cell):
    """floor((v + o) / cell) in double, or None where that is not finite or does not fit an int32."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        f = np.floor((np.float64(v) + np.float64(o)) / np.float64(cell))
    return int(f) if np.isfinite(f) and -2147483648.0 <= f <= 2147483647.0 else None


def path_cells(bool_map, start_xy, goal_xy, cell=0.1, ox=1.0, oy=1.0, height_bound=0.2, max_cells=None, max_open=PATH_MAX_OPEN):
    """``PathSolver.astar`` on arrays.  Returns (cells [max_cells, 2] int32 (row, col), padding 0; n_cells; status).
    The start and goal cells are (floor((y + oy) / cell), floor((x + ox) / cell)) in double.  Per cell of the grid: g (an
    integer: every step costs exactly 1.0; 0 where ``gscore.get(nb, 0)`` finds nothing), the direction it was reached by, a
    closed bit and the number of its entries in the open list, which is an unsorted array of (f, row * cols + col) popped by an
    exact lexicographic minimum (heapq's order: equal tuples are indistinguishable, and only cells inside the grid are ever
    pushed).  The start cell is the list's only first entry: it is expanded without being indexed, so it may lie outside the
    grid.  f = g + sqrt(dr * dr + dc * dc) with dr, dc exact and every other operation one rounded double operation.
    status 0 found; 1 no path (the open list ran empty, or a start / goal cell that is not finite or no int32); 2 the path has
    more than max_cells cells (n_cells is then its length, cells stay 0); 3 a push would make the open list longer than
    max_open, or more than 4 * rows * cols + 4 pops happened."""
    m = np.asarray(bool_map)
    rows, cols = m.shape
    max_cells = rows * cols + 1 if max_cells is None else int(max_cells)
    cells = np.zeros((max_cells, 2), np.int32)
    sr, sc = _cell_of(start_xy[1], oy, cell), _cell_of(start_xy[0], ox, cell)
    gr, gc = _cell_of(goal_xy[1], oy, cell), _cell_of(goal_xy[0], ox, cell)
    if None in (sr, sc, gr, gc):
        return cells, 0, 1
    blocked = m > height_bound
    g = np.zeros((rows, cols), np.int64)
    came = np.zeros((rows, cols), np.int64)
    closed = np.zeros((rows, cols), bool)
    live = np.zeros((rows, cols), np.int64)
    of, oc, n_open = np.empty(max_open), np.empty(max_open, np.int64), 0
    inside = lambda r, c: 0 <= r < rows and 0 <= c < cols
    cur, pops = (sr, sc), 0
    while True:
        if pops > 0:                                       # (the first pop is the start: the list's only entry)
            if n_open == 0:
                return cells, 0, 1
            fmin = of[:n_open].min()
            cand = np.flatnonzero(of[:n_open] == fmin)
            k = cand[np.argmin(oc[cand])]
            cur = (int(oc[k]) // cols, int(oc[k]) % cols)
            n_open -= 1
            of[k], oc[k] = of[n_open], oc[n_open]          # swap with the last
            live[cur] -= 1
        pops += 1
        if pops > 4 * rows * cols + 4:
            return cells, 0, 3
        if cur == (gr, gc):
            break
        gcur = 0
        if inside(*cur):
            closed[cur] = True
            gcur = int(g[cur])
        for d, (di, dj) in enumerate(PATH_NEIGHBOURS):
            nb = (cur[0] + di, cur[1] + dj)
            if not inside(*nb) or blocked[nb]:
                continue
            gn = gcur + 1
            if closed[nb] and gn >= g[nb]:
                continue
            if gn < g[nb] or live[nb] == 0:
                if n_open >= max_open:
                    return cells, 0, 3
                came[nb], g[nb] = d, gn
                dr, dc = np.float64(gr - nb[0]), np.float64(gc - nb[1])
                of[n_open], oc[n_open] = np.float64(gn) + np.sqrt(dr * dr + dc * dc), nb[0] * cols + nb[1]
                n_open += 1
                live[nb] += 1
    back = []                                              # ``while current in came_from``: inside the grid and reached by a step
    while inside(*cur) and g[cur] > 0:
        back.append(cur)
        di, dj = PATH_NEIGHBOURS[came[cur]]
        cur = (cur[0] - di, cur[1] - dj)
    n_cells = len(back) + 1
    if n_cells > max_cells:
        return cells, n_cells, 2
    cells[0] = (sr, sc)
    if back:
        cells[1:n_cells] = back[::-1]
    return cells, n_cells, 0


def spine_fit(t, y):
    """The not-a-knot cubic through the n + 1 points (t[i], y[i]) as c [4, n] in scipy's ``CubicSpline.c`` layout, by a fixed
    sequence of double operations.  h[i] = t[i + 1] - t[i], d[i] = (y[i + 1] - y[i]) / h[i]; the knot slopes s are
      n = 1: s = (d[0], d[0]): the line
      n = 2: scipy's 3 x 3 system [1 1 0; h1 2(h0 + h1) h0; 0 1 1] s = (2 d0, 3 (h0 d1 + h1 d0), 2 d1) with s0 and s2 eliminated:
             s1 = ((b1 - h1 b0) - h0 b2) / ((2 (h0 + h1) - h1) - h0), s0 = b0 - s1, s2 = b2 - s1: the parabola
      n >= 3: scipy's tridiagonal system (rows h[i], 2 (h[i - 1] + h[i]), h[i - 1]; the two not-a-knot end rows) by the Thomas
             recurrence without pivoting: c'[0] = u0 / d0, g'[0] = b0 / d0, den = d[i] - l[i] c'[i - 1], c'[i] = u[i] / den,
             g'[i] = (b[i] - l[i] g'[i - 1]) / den, then s[n] = g'[n], s[i] = g'[i] - c'[i] s[i + 1]
    and then scipy's last lines: t = (s[i] + s[i + 1] - 2 d[i]) / h[i], c0 = t / h[i], c1 = (d[i] - s[i]) / h[i] - t, c2 = s[i],
    c3 = y[i]."""
    t, y = np.asarray(t, np.float64), np.asarray(y, np.float64)
    n = len(t) - 1
    if n < 1 or len(y) != n + 1:
        raise ValueError("spine_fit needs two points at least, and as many values as knots")
    two, three = np.float64(2.0), np.float64(3.0)
    with np.errstate(all="ignore"):
        h = [t[i + 1] - t[i] for i in range(n)]
        d = [(y[i + 1] - y[i]) / h[i] for i in range(n)]
        if n == 1:
            s = [d[0], d[0]]
        elif n == 2:
            b0, b1, b2 = two * d[0], three * (h[0] * d[1] + h[1] * d[0]), two * d[1]
            s1 = ((b1 - h[1] * b0) - h[0] * b2) / ((two * (h[0] + h[1]) - h[1]) - h[0])
            s = [b0 - s1, s1, b2 - s1]
        else:
            cp, gp = [None] * n, [None] * (n + 1)
            dd = t[2] - t[0]
            b = ((h[0] + two * dd) * h[1] * d[0] + h[0] * h[0] * d[1]) / dd
            cp[0], gp[0] = dd / h[1], b / h[1]
            for i in range(1, n):
                b = three * (h[i] * d[i - 1] + h[i - 1] * d[i])
                den = two * (h[i - 1] + h[i]) - h[i] * cp[i - 1]
                cp[i], gp[i] = h[i - 1] / den, (b - h[i] * gp[i - 1]) / den
            dd = t[n] - t[n - 2]
            b = (h[n - 1] * h[n - 1] * d[n - 2] + (two * dd + h[n - 1]) * h[n - 2] * d[n - 1]) / dd
            den = h[n - 2] - dd * cp[n - 1]
            gp[n] = (b - dd * gp[n - 1]) / den
            s = gp
            for i in range(n - 1, -1, -1):
                s[i] = gp[i] - cp[i] * s[i + 1]
        c = np.zeros((4, n))
        for i in range(n):
            tt = ((s[i] + s[i + 1]) - two * d[i]) / h[i]
            c[0, i], c[1, i], c[2, i], c[3, i] = tt / h[i], (d[i] - s[i]) / h[i] - tt, s[i], y[i]
    return c


PATH_PLAN_FIELDS = ("rows", "cols", "cell", "origin_x", "origin_y", "height_bound", "step_size", "max_cells", "max_open", "max_pieces",
                    "n_maps", "set_done")


def path_plan(maps, map_id, start, goal, params, done=None):
    """The global paths of B windows as the table ``path_goal`` reads: the rule of k_path_plan.  maps [n_maps, rows, cols] (or
    [rows, cols]) boolean maps (blocked: > height_bound) with map_id [B] (None: map 0; ids outside are read as the nearest
    map); start [B, >= 2] the windows' start points (x, y); goal [B, 3] the robots' goals; params: a ``capi.QtosPathPlan`` or a
    dict of cell, origin_x, origin_y, height_bound, step_size, max_cells, max_open, max_pieces, set_done.  Per window, as
    ``PathSolver``: ``path_cells``; sub = path[::2], n = len(sub) pieces; xs = col * cell - origin_x over sub, then the last
    cell's col * cell WITHOUT the shift (sic); ys likewise from the rows; T = sqrt(dx dx + dy dy) / step_size * 10 from the
    start and goal coordinates; knots i * (T / n), the last one T (numpy's linspace); ``spine_fit`` twice.  A window whose
    status is not 0, or whose T is not > 0 (status 4), gets the one-piece constant spine at its start point over the knots
    (0, 0).  Rows are padded as ``path_table`` pads them, to max_pieces.  Returns the dict of ``path_table`` (knots, coef,
    n_pieces, robot_goal) plus cells [B, max_cells, 2], n_cells [B], status [B] (int32), and done [B] where ``done`` is
    given: with set_done, bit 2 (value 4) is set in it where the status is not 0."""
    g = lambda name: _path_param(params, name)
    m = np.asarray(maps)
    m = m[None] if m.ndim == 2 else m
    start = np.asarray(start, np.float64)
    B = len(start)
    start = start.reshape(B, -1)
    rg = np.asarray(goal, np.float64).reshape(B, 3)
    mid = np.zeros(B, np.int64) if map_id is None else np.clip(np.asarray(map_id, np.int64).reshape(B), 0, len(m) - 1)
    cell, ox, oy = np.float64(g("cell")), np.float64(g("origin_x")), np.float64(g("origin_y"))
    step, ten = np.float64(g("step_size")), np.float64(10.0)
    max_cells, max_open, mp = int(g("max_cells")), int(g("max_open")), int(g("max_pieces"))
    if m.shape[1] * m.shape[2] > PATH_MAX_GRID or not 1 <= max_open <= PATH_MAX_OPEN or not 1 <= max_cells <= 2 * mp:
        raise ValueError("rows * cols <= %d, 1 <= max_open <= %d and 1 <= max_cells <= 2 * max_pieces" % (PATH_MAX_GRID, PATH_MAX_OPEN))
    knots, coef = np.zeros((B, mp + 1)), np.zeros((B, 2, 4, mp))
    n_pieces = np.ones(B, np.int32)
    cells, n_cells, status = np.zeros((B, max_cells, 2), np.int32), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        cells[b], n_cells[b], status[b] = path_cells(m[mid[b]], start[b, 0:2], rg[b, 0:2], cell, ox, oy, g("height_bound"), max_cells,
                                                     max_open)
        with np.errstate(all="ignore"):
            dx, dy = start[b, 0] - rg[b, 0], start[b, 1] - rg[b, 1]
            T = np.sqrt(dx * dx + dy * dy) / step * ten
            if status[b] == 0 and not T > 0:
                status[b] = 4
            if status[b] != 0:
                coef[b, 0, 3, 0], coef[b, 1, 3, 0] = start[b, 0], start[b, 1]
                continue
            path = cells[b, :n_cells[b]].astype(np.int64)
            sub = path[::2]
            n = len(sub)
            xs = np.append(sub[:, 1] * cell - ox, path[-1, 1] * cell)
            ys = np.append(sub[:, 0] * cell - oy, path[-1, 0] * cell)
            t = np.arange(n + 1) * (T / np.float64(n))
            t[n] = T
        n_pieces[b] = n
        knots[b, :n + 1], knots[b, n + 1:] = t, T
        coef[b, 0, :, :n], coef[b, 1, :, :n] = spine_fit(t, xs), spine_fit(t, ys)
    out = dict(knots=knots, coef=coef, n_pieces=n_pieces, robot_goal=rg.copy(), cells=cells, n_cells=n_cells, status=status)
    if done is not None:
        out["done"] = np.asarray(done, np.int32).reshape(B) | np.where((status != 0) & bool(g("set_done")), PATH_DONE_BIT, 0).astype(np.int32)
    return out
