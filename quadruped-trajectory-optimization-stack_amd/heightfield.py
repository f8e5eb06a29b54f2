"""Terrain files: the side channel between QTOS's map generator and the solver.

Counterpart of QTOS/generateHeightField.py: tile reader (:100-118, tiles are read transposed),
nearest-neighbour upsampling (:39-56), tile concatenation along x (:470-484), the solver's copy
(transpose, shifted one row toward +x: :568,620-631) and the text format
(``"v, v, ..., v,"`` per line, no final newline: :590-605), the height-level randomiser
(:692-730), the random shifts (:648-690), the randomised terrain of ``randomize_env`` (:563-567: ``random_env``) and
``random_env_table``, the statement of that rule in arrays and integers which the device kernel k_terrain_env equals to the bit.
World frame: map index (row = y, col = x), cell = 2 / rows metres, origin shift 1.0 in x and y
(QTOS/planner.py:61-62), i.e. x in [-1, 2*tiles - 1], y in [-1, 1].
"""
import numpy as np


def read_tile(path, delimiter=','):
    rows = []
    with open(path) as f:
        for line in f.readlines():
            vals = []
            for tok in line.strip().split(delimiter):
                try:
                    vals.append(float(tok))
                except ValueError:
                    pass
            rows.append(vals)
    return np.transpose(np.array(rows))


def scale_map(tile, scale_factor=1):
    return np.repeat(np.repeat(np.asarray(tile), scale_factor, axis=0), scale_factor, axis=1)


def build_map(tiles, mesh_scale=1):
    """List of tile arrays (as read_tile returns them) -> map[y_index][x_index]."""
    return np.concatenate([scale_map(t, mesh_scale) for t in tiles], axis=1)


def towr_map(map_yx):
    """The array the reference writes for the solver: [x_index][y_index], shifted one row in +x."""
    m = np.transpose(np.array(map_yx, dtype=float))
    out = np.zeros_like(m)
    out[1:] = m[:-1]
    return out


def random_height(map_yx, rng, height_delta=0.005):
    """One pass of the reference's terrain randomiser (QTOS/generateHeightField.py:708-730): every
    distinct non-zero height level (ascending) moves as a whole by +d, -d or not at all, d uniform
    in [-height_delta, height_delta].  `rng` is a `random.Random`; seeded like the module-level
    generator the reference uses it reproduces the reference's maps (tests/golden/random_height.json)."""
    out = np.array(map_yx, dtype=float)
    for h in np.unique(out[out != 0]):
        d = rng.uniform(-height_delta, height_delta)
        n = rng.choice((0, 1, 2))
        if n == 0:
            out[out == h] += d
        elif n == 1:
            out[out == h] -= d
    return out


def random_height_shift(map_yx, shift, rng):
    """`shift` cumulative passes of random_height (QTOS/generateHeightField.py:692-706; the
    reference's randomize_env applies 10)."""
    out = np.array(map_yx, dtype=float)
    for _ in range(shift):
        out = random_height(out, rng)
    return out


DIRECTIONS = ("left", "right", "up", "down")       # (dy, dx) of a step: left is -1 on axis 1, up is -1 on axis 0
STEP = {"left": (0, -1), "right": (0, 1), "up": (-1, 0), "down": (1, 0)}


def random_map_shift(map_yx, shift, rng, climb=False):
    """`shift` cumulative steps of the reference's shift_map (QTOS/generateHeightField.py:648-690): each rolls the array by one
    cell with wrap-around in a direction `rng.choice` picks, from left / right / up / down, or from up / down alone on a climb
    map (climb_map_check).  `rng` is a `random.Random`."""
    out = np.array(map_yx, dtype=float)
    directions = DIRECTIONS[2:] if climb else DIRECTIONS
    for _ in range(shift):
        dy, dx = STEP[rng.choice(directions)]
        out = np.roll(out, shift=dy if dy else dx, axis=0 if dy else 1)
    return out


def random_env(map_yx, rng, shift=10, height=10, climb=False):
    """The terrain `Height_Map_Generator(randomize_env=True)` leaves in `self.map` (QTOS/generateHeightField.py:563-567): the
    reference's four calls in its order -- shifts of the solver's copy, shifts of the map, height passes of the solver's copy,
    height passes of the map -- on one stream.  The solver's copy is rebuilt from the map afterwards (:568), so only the
    draws it consumes matter.  shift: random_shift_num * mesh_scale (the reference's 10 * mesh_scale)."""
    m = np.array(map_yx, dtype=float)
    towr = random_map_shift(np.transpose(m), shift, rng, climb)
    m = random_map_shift(m, shift, rng, climb)
    random_height_shift(towr, height, rng)
    return random_height_shift(m, height, rng)


ENV_MAX_LEVELS = 64          # QTOS_ENV_MAX_LEVELS
ENV_MAX_DRAWS = 1 << 24      # draws[m] on entry


class MT19937:
    """Python's `random.Random(seed)` for 0 <= seed < 2**64 from scratch, in integers: the generator, CPython's seeding
    (init_by_array on the seed's 32-bit words, low word first: one word below 2**32, two below 2**64) and its `random`,
    `uniform` and `choice` arithmetic.  `draws` counts the 32-bit outputs consumed."""

    def __init__(self, seed, skip=0):
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed is 0 .. 2**64 - 1")
        key = [seed & 0xffffffff] + ([seed >> 32] if seed >> 32 else [])
        mt = [0] * 624
        mt[0] = 19650218
        for i in range(1, 624):
            mt[i] = (1812433253 * (mt[i - 1] ^ (mt[i - 1] >> 30)) + i) & 0xffffffff
        i, j = 1, 0
        for _ in range(624):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1664525)) + key[j] + j) & 0xffffffff
            i, j = i + 1, (j + 1) % len(key)
            if i >= 624:
                mt[0], i = mt[623], 1
        for _ in range(623):
            mt[i] = ((mt[i] ^ ((mt[i - 1] ^ (mt[i - 1] >> 30)) * 1566083941)) - i) & 0xffffffff
            i += 1
            if i >= 624:
                mt[0], i = mt[623], 1
        mt[0] = 0x80000000
        self.mt, self.pos, self.draws = np.array(mt, np.uint32), 624, 0
        while skip - self.draws >= 624 - self.pos:         # whole states are skipped without tempering them
            self.draws += 624 - self.pos
            self._twist()
        self.pos += skip - self.draws
        self.draws = skip

    def _twist(self):
        """The next 624 words, in the three runs whose words do not depend on one another: [0, 227), [227, 454), [454, 623]."""
        mt = self.mt

        def mix(a, b):
            y = (a & np.uint32(0x80000000)) | (b & np.uint32(0x7fffffff))
            return (y >> np.uint32(1)) ^ ((y & np.uint32(1)) * np.uint32(0x9908b0df))
        mt[0:227] = mt[397:624] ^ mix(mt[0:227], mt[1:228])
        mt[227:454] = mt[0:227] ^ mix(mt[227:454], mt[228:455])
        mt[454:623] = mt[227:396] ^ mix(mt[454:623], mt[455:624])
        mt[623] = mt[396] ^ mix(mt[623], mt[0])
        self.pos = 0

    def bits32(self):
        if self.pos >= 624:
            self._twist()
        y = int(self.mt[self.pos])
        self.pos += 1
        self.draws += 1
        y ^= y >> 11
        y ^= (y << 7) & 0x9d2c5680
        y ^= (y << 15) & 0xefc60000
        return y ^ (y >> 18)

    def random(self):
        a, b = self.bits32() >> 5, self.bits32() >> 6
        return np.float64(a * 67108864 + b) / np.float64(9007199254740992.0)

    def uniform(self, a, b):
        a, b = np.float64(a), np.float64(b)
        return a + (b - a) * self.random()                 # (two roundings: the product, then the sum)

    def below(self, n):
        """Index of `choice` among n items: the top bit_length(n) bits of an output, redrawn while >= n."""
        k = int(n).bit_length()
        r = self.bits32() >> (32 - k)
        while r >= n:
            r = self.bits32() >> (32 - k)
        return r


def _level_pass(vals, mt, delta):
    """One pass of random_height on the list of level values (in place): the snapshot of the ascending distinct values != 0,
    and per snapshot level h a draw of d and of the choice, applied to every entry that equals h as the list stands then."""
    for h in np.unique(vals[vals != 0]):
        d = mt.uniform(-delta, delta)
        c = mt.below(3)
        if c == 0:
            vals[vals == h] += d
        elif c == 1:
            vals[vals == h] -= d


def random_env_table(base_yx, seed, draws=None, base_id=None, n_shift=10, n_height=10, climb=False, delta=0.005, fill=0.0):
    """The rule of k_terrain_env (qtos_terrain_env*), stated in numpy and Python integers; the kernel equals it to the bit, and
    tests/test_terrain_env_cpu.py holds it to the reference's `random_env` sequence.

    base_yx [n_base, rows, cols] (or [rows, cols]); seed [n_maps] (0 .. 2**64 - 1); draws [n_maps]: 32-bit outputs of the map's
    stream already consumed (None: 0); base_id [n_maps]: the base grid map m starts from (None: map m reads base m).  Per map:
    the stream of `random.seed(seed[m])` behind its first draws[m] outputs; n_shift `choice`s of a direction for the solver's
    copy (consumed, no effect) and n_shift for the map, whose rolls are one net roll (dy, dx); n_height height passes of the
    solver's copy -- on its list of levels alone -- and n_height of the map.  A level is a distinct value != 0 of the grid
    (-0.0 is ground); every cell belongs to the level slot it starts in, and a pass moves whole slots.

    Returns dict(map_yx [n_maps, rows, cols], height_xy [n_maps, cols, rows] = towr_map(map_yx), draws [n_maps] int32 moved on,
    status [n_maps] int32, net_shift [n_maps, 2]).  status: 0 ok; 2 draws[m] negative or > 2**24 on entry; 4 base_id[m] outside
    0 .. n_base - 1; 3 a NaN in the base grid; 1 more than 64 distinct levels (checked in that order: 2, 4, 3, 1).  A map with a
    non-zero status keeps `fill` in both grids and its draws."""
    base = np.asarray(base_yx, dtype=float)
    base = base[None] if base.ndim == 2 else base
    seed = [int(s) for s in np.ravel(seed)]
    n_maps, (rows, cols) = len(seed), base.shape[1:]
    draws = np.zeros(n_maps, np.int32) if draws is None else np.array(draws, np.int32).reshape(n_maps)
    base_id = np.arange(n_maps) if base_id is None else np.asarray(base_id).reshape(n_maps)
    out = dict(map_yx=np.full((n_maps, rows, cols), fill, float), height_xy=np.full((n_maps, cols, rows), fill, float),
               draws=draws.copy(), status=np.zeros(n_maps, np.int32), net_shift=np.zeros((n_maps, 2), np.int64))
    n_dir = 2 if climb else 4
    for m in range(n_maps):
        if draws[m] < 0 or draws[m] > ENV_MAX_DRAWS:
            out["status"][m] = 2
            continue
        if not 0 <= base_id[m] < len(base):
            out["status"][m] = 4
            continue
        grid = base[base_id[m]]
        if np.isnan(grid).any():
            out["status"][m] = 3
            continue
        levels = np.unique(grid[grid != 0])
        if len(levels) > ENV_MAX_LEVELS:
            out["status"][m] = 1
            continue
        mt = MT19937(seed[m], int(draws[m]))
        for _ in range(n_shift):
            mt.below(n_dir)
        dy = dx = 0
        for _ in range(n_shift):
            sy, sx = STEP[DIRECTIONS[mt.below(n_dir) + (2 if climb else 0)]]
            dy, dx = dy + sy, dx + sx
        solver, vals = levels.copy(), levels.copy()
        for _ in range(n_height):
            _level_pass(solver, mt, delta)
        for _ in range(n_height):
            _level_pass(vals, mt, delta)
        moved, on_level = grid.copy(), grid != 0           # (ground cells keep their own value, -0.0 included)
        moved[on_level] = vals[np.searchsorted(levels, grid[on_level])]
        out["map_yx"][m] = np.roll(np.roll(moved, dy, axis=0), dx, axis=1)
        out["height_xy"][m] = towr_map(out["map_yx"][m])
        out["draws"][m] = mt.draws
        out["net_shift"][m] = (dy, dx)
    return out


def cell_size(map_yx):
    return 1.0 / (np.asarray(map_yx).shape[0] / 2.0)


def write_height_file(path, arr):
    rows = len(arr)
    with open(path, 'w') as f:
        for k, line in enumerate(arr):
            f.write(', '.join(str(v) for v in line) + ',')
            if k < rows - 1:
                f.write('\n')


def read_height_file(path):
    """Solver-side reader of the same format -> float array [x_index][y_index]."""
    rows = []
    with open(path) as f:
        for line in f.read().split('\n'):
            vals = [float(t) for t in line.split(',') if t.strip() != '']
            if vals:
                rows.append(vals)
    return np.array(rows)


def height_at(height_xy, cell, x, y, x0=-1.0, y0=-1.0, mode=0):
    """Terrain height as the planner kernels evaluate it: mode 0 bilinear (clamped at the border),
    mode 1 nearest cell."""
    h = np.asarray(height_xy, float)
    fx = np.clip((np.asarray(x, float) - x0) / cell, 0, h.shape[0] - 1)
    fy = np.clip((np.asarray(y, float) - y0) / cell, 0, h.shape[1] - 1)
    if mode == 1:
        return h[np.floor(fx + 0.5).astype(int), np.floor(fy + 0.5).astype(int)]
    ix = np.clip(np.floor(fx).astype(int), 0, max(h.shape[0] - 2, 0))
    iy = np.clip(np.floor(fy).astype(int), 0, max(h.shape[1] - 2, 0))
    ix1 = np.minimum(ix + 1, h.shape[0] - 1)
    iy1 = np.minimum(iy + 1, h.shape[1] - 1)
    u, v = fx - ix, fy - iy
    return (h[ix, iy] * (1 - u) * (1 - v) + h[ix1, iy] * u * (1 - v)
            + h[ix, iy1] * (1 - u) * v + h[ix1, iy1] * u * v)
