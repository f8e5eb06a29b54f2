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
