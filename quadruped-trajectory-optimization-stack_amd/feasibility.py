"""Batched feasibility map: counterpart of QTOS/generateHeightField.py ``PATH_MAP`` (:172-404).

The reference enumerates (start, goal) patches two cells apart next to obstacles, runs ONE solver
process per patch in 32 OS processes and keeps only the exit codes.  Here the patches are
enumerated the same way (``probe_patches`` reproduces ``probe_map`` incl. its rounding and index
walk), solved as ONE GPU batch, and the statuses are stamped into the boolean map with the same
rules: success clears the start / middle / goal cells, failure stamps the diamond-shaped
neighbourhood of the start and goal cells (the reference's "mid" stamp is a no-op, :397-399).
"""
import numpy as np


def neighbors_danger_test(m, ix, iy, sz=1):
    nb = ((sz, 0), (-sz, 0), (0, sz), (0, -sz), (sz, sz), (sz, -sz), (-sz, -sz), (-sz, sz))
    for dx, dy in nb:
        if dx + ix >= m.shape[0] or dx + ix < 0:
            return False
        elif dy + iy >= m.shape[1] or dy + iy < 0:
            return False
        elif m[dx + ix][dy + iy] > 0:
            return True
    return False


def probe_patches(m, multi_map_shift=1, res=0.1, origin_shift=1.0):
    """List of (start_xyz, goal_xyz, start_idx, goal_idx) exactly as ``PATH_MAP.probe_map`` queues them."""
    m = np.asarray(m)
    step = res
    x_start = -res * (m.shape[1] / 2) - res / 2 + ((multi_map_shift - 1) * origin_shift)
    y_start = -res * (m.shape[1] / 2) - res / 2 + ((multi_map_shift - 1) * origin_shift)
    x_goal = -res * (m.shape[1] / 2) + res / 2 + ((multi_map_shift - 1) * origin_shift)
    y_goal = -res * (m.shape[1] / 2) - res / 2 + ((multi_map_shift - 1) * origin_shift)
    _x_start, _y_start, _x_goal, _y_goal = x_start, y_start, x_goal, y_goal
    ix, iy, iy2 = 0, 0, 2
    out = []
    for _ in range(m.shape[0]):
        _y_start += step
        _y_goal += step
        _x_start, _x_goal = x_start, x_goal
        for y in range(m.shape[1] // 2 - 1):
            if y == 0:
                _x_start += step
                iy, iy2 = 0, 2
            else:
                _x_start = _x_goal
            _x_goal += 2 * step
            _x_start, _y_start = round(_x_start, 2), round(_y_start, 2)
            _x_goal, _y_goal = round(_x_goal, 2), round(_y_goal, 2)
            if neighbors_danger_test(m, ix, iy) or neighbors_danger_test(m, ix, iy2):
                out.append(((_x_start, _y_start, float(m[ix][iy])), (_x_goal, _y_goal, float(m[ix][iy2])),
                            (ix, iy), (ix, iy2)))
            iy += 2
            iy2 += 2
        ix += 1
    return out


def diamond(scale=1):
    """Cells of the hull of ((-3s,0),(3s,0),(0,-3s),(0,3s)) relative to its centre
    (``find_convex_hull``): |dx| + |dy| <= 3 s, row-major order."""
    r = 3 * scale
    return [(a, b) for a in range(-r, r + 1) for b in range(-r, r + 1) if abs(a) + abs(b) <= r]


def patch_args(start_pt, goal_pt):
    """Solver flags of one patch (``worker_f.state_config``, :365-373)."""
    shift = np.array([start_pt[0], start_pt[1], start_pt[2]])
    return {'-s': [start_pt[0], start_pt[1], start_pt[2] + 0.24],
            '-e1': (np.array([0.21, 0.19, 0.0]) + shift).tolist(),
            '-e2': (np.array([0.21, -0.19, 0.0]) + shift).tolist(),
            '-e3': (np.array([-0.21, 0.19, 0.0]) + shift).tolist(),
            '-e4': (np.array([-0.21, -0.19, 0.0]) + shift).tolist(),
            '-s_ang': [0, 0, 0], '-g': [goal_pt[0], goal_pt[1], goal_pt[2] + 0.24], '-r': 5.0}


def stamp(shape, patches, statuses, scale=1):
    """Exit codes -> boolean map (``worker_f``, :387-404), patches processed in queue order."""
    bm = np.zeros(shape, dtype=int)
    hull = diamond(scale)
    for (_, _, s_idx, g_idx), rc in zip(patches, statuses):
        if rc == 0:
            bm[s_idx] = 0
            bm[s_idx[0], s_idx[1] + 1] = 0
            bm[g_idx] = 0
        else:
            for c in (s_idx, g_idx):
                for a, b in hull:
                    if 0 <= c[0] + a < shape[0] and 0 <= c[1] + b < shape[1]:
                        bm[c[0] + a, c[1] + b] = 1
    return bm


def feasibility_map(local_planner, map_yx, multi_map_shift=1, scale=1):
    """One batched solve over every probe patch -> (bool_map, patches, statuses)."""
    m = np.asarray(map_yx)
    if np.all(m == 0):
        return np.zeros(m.shape, dtype=int), [], []     # check_flat_ground short-cut (:222-225)
    patches = probe_patches(m, multi_map_shift, 0.1 * (1 / scale))
    statuses = local_planner.solve_batch([patch_args(p[0], p[1]) for p in patches], sample=False)
    return stamp(m.shape, patches, statuses, scale), patches, statuses


# ---- the probe and the stamp of n_maps maps as arrays: the rule of k_probe / k_probe_stamp (qtos_probe*) in numpy ----------
# ``probe_patches`` and ``stamp`` above walk one map in Python loops; the functions below state the same rule over a stack of
# maps as arrays, every coordinate formed by the same rounded double operations in the same order, and the kernels equal them
# to the bit (as ``global_planner.path_plan`` is the statement of k_path_plan).

NOMINAL_STANCE = ((0.21, 0.19, 0.0), (0.21, -0.19, 0.0), (-0.21, 0.19, 0.0), (-0.21, -0.19, 0.0))   # FL FR HL HR (patch_args)
Z_OFFSET = 0.24
_NEIGHBOURS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (1, -1), (-1, -1), (-1, 1))                # neighbors_danger_test, sz = 1
_SPLIT = 134217729.0                                                                               # 2^27 + 1 (Veltkamp)


def _product_error(a, b, p):
    """a * b - p exactly, p = fl(a * b) (Dekker's product; what fma(a, b, -p) returns)."""
    c = _SPLIT * a
    ah = c - (c - a)
    al = a - ah
    c = _SPLIT * b
    bh = c - (c - b)
    bl = b - bh
    return ((ah * bh - p) + ah * bl + al * bh) + al * bl


def round2(v):
    """Python's ``round(v, 2)`` on doubles (a scalar or an array): p = v * 100 with its exact error e, k = rint(p), and where p
    lies exactly half way between two integers although the true product does not (e != 0) the side the true product lies on;
    k / 100.  A true tie (e = 0) goes to the even k, as ``round`` does.  For |v| < 2^52 / 100."""
    a = np.asarray(v, np.float64)
    p = a * 100.0
    e = _product_error(a, np.float64(100.0), p)
    k = np.rint(p)
    f = np.floor(p)
    k = np.where((np.abs(p - k) == 0.5) & (e != 0.0), f + (e > 0.0), k)
    out = k / 100.0
    return out if out.ndim else float(out)


def _danger(maps):
    """``neighbors_danger_test`` of every cell of every map: the first neighbour outside the map answers False, the first inside
    it that is > 0 answers True (a NaN is not > 0)."""
    n_maps, rows, cols = maps.shape
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    danger = np.zeros(maps.shape, bool)
    open_ = np.ones((rows, cols), bool)                    # (no neighbour has answered yet)
    for dr, dc in _NEIGHBOURS:
        inside = (r + dr >= 0) & (r + dr < rows) & (c + dc >= 0) & (c + dc < cols)
        val = maps[:, np.clip(r + dr, 0, rows - 1), np.clip(c + dc, 0, cols - 1)]
        with np.errstate(invalid="ignore"):
            hit = (open_ & inside)[None] & (val > 0)
        danger |= hit                                      # (only ever set: a cell that answered True stays True)
        open_ = open_ & inside
    return danger


def probe_table(maps_yx, multi_map_shift=1, scale=1, origin_shift=1.0, cell=0.1):
    """The probe patches of n_maps maps (n_maps x rows x cols, or rows x cols) in queue order -- per map those of
    ``probe_patches(m, multi_map_shift, cell * (1 / scale), origin_shift)``, map 0's first -- as a dict of arrays:
    offsets [n_maps + 1] int32 (exclusive prefix sums, offsets[-1] = N), slot [n_maps, rows, cols // 2 - 1] int32 (a patch's
    index, or -1), patch [N, 3] int32 (map, row, start column), start [N, 24], goal [N, 3] (the bits of
    ``flags.problem_arrays(patch_args(...))``) and map_id [N] int32."""
    maps = np.asarray(maps_yx, np.float64)
    maps = maps[None] if maps.ndim == 2 else maps
    n_maps, rows, cols = maps.shape
    nj = max(cols // 2 - 1, 0)
    res = cell * (1 / scale)
    shift = (multi_map_shift - 1) * origin_shift
    x_start = ((-res * (cols / 2)) - res / 2) + shift      # (sic: both start values use shape[1])
    y_start = ((-res * (cols / 2)) - res / 2) + shift
    x_goal = ((-res * (cols / 2)) + res / 2) + shift
    ys = np.zeros(rows)
    y = y_start
    for r in range(rows):
        y = round2(y + res)
        ys[r] = y
    xs = np.zeros(nj + 1)                                  # xs[j] starts patch j, xs[j + 1] is its goal
    if nj:
        xs[0] = round2(x_start + res)
        xg = x_goal
        for j in range(nj):
            xg = round2(xg + 2 * res)
            xs[j + 1] = xg
    danger = _danger(maps)
    cand = danger[:, :, 0:2 * nj:2] | danger[:, :, 2:2 * nj + 2:2] if nj else np.zeros((n_maps, rows, 0), bool)
    count = cand.reshape(n_maps, -1).sum(axis=1)
    offsets = np.concatenate([[0], np.cumsum(count)]).astype(np.int32)
    N = int(offsets[-1])
    slot = np.where(cand, np.cumsum(cand.ravel()).reshape(cand.shape) - 1, -1).astype(np.int32)
    mi, ri, ji = np.nonzero(cand)                          # (C order: map, row, j -- the queue order)
    patch = np.stack([mi, ri, 2 * ji], axis=1).astype(np.int32).reshape(N, 3)
    z, zg = maps[mi, ri, 2 * ji], maps[mi, ri, 2 * ji + 2]
    px, py = xs[ji], ys[ri]
    start = np.zeros((N, 24))
    start[:, 0], start[:, 1], start[:, 2] = px, py, z + Z_OFFSET
    for e, (fx, fy, fz) in enumerate(NOMINAL_STANCE):
        start[:, 6 + 3 * e], start[:, 7 + 3 * e], start[:, 8 + 3 * e] = fx + px, fy + py, fz + z
    goal = np.stack([xs[ji + 1], py, zg + Z_OFFSET], axis=1).reshape(N, 3)
    return dict(offsets=offsets, slot=slot, patch=patch, start=start, goal=goal, map_id=mi.astype(np.int32))


def stamp_table(shape, offsets, slot, patch, status, scale=1):
    """``stamp`` over all maps: n_maps x rows x cols doubles of 0.0 / 1.0, the ``bool_maps`` of ``qtos_path_plan*``.  shape
    (rows, cols) or (n_maps, rows, cols).  A cell holds what the LAST patch in queue order that writes it leaves: status 0
    writes 0 to the start cell, the cell right of it and the goal cell, any other status 1 to the diamonds |a| + |b| <= 3 scale
    round the start and the goal cell, clipped to the map; a cell nothing writes is 0.  (slot is the kernel's way to the patches
    near a cell; the statement goes through the patches and needs only its shape.)"""
    offsets, patch, status = np.asarray(offsets), np.asarray(patch).reshape(-1, 3), np.asarray(status).reshape(-1)
    n_maps = len(offsets) - 1
    rows, cols = tuple(shape)[-2:]
    N = int(offsets[-1])
    if np.shape(slot)[:2] != (n_maps, rows) or len(patch) < N or len(status) < N:
        raise ValueError("slot is n_maps x rows x (cols // 2 - 1); patch and status hold offsets[-1] entries")
    last = np.full((n_maps, rows, cols), -1, np.int64)     # per cell: the last patch that writes it
    idx = np.arange(N)
    pm, pr, pc = patch[:N, 0], patch[:N, 1], patch[:N, 2]
    ok, bad = status[:N] == 0, status[:N] != 0
    for dc in (0, 1, 2):
        np.maximum.at(last, (pm[ok], pr[ok], pc[ok] + dc), idx[ok])
    for a, b in diamond(scale):
        for c0 in (0, 2):
            r, c = pr + a, pc + c0 + b
            w = bad & (r >= 0) & (r < rows) & (c >= 0) & (c < cols)
            np.maximum.at(last, (pm[w], r[w], c[w]), idx[w])
    out = np.zeros((n_maps, rows, cols))
    out[last >= 0] = (status[:N][last[last >= 0]] != 0).astype(np.float64)
    return out


def feasibility_maps_device(planner, maps_yx, multi_map_shift=1, scale=1, stream=None):
    """``feasibility_map`` of n_maps maps without a host loop: k_probe lists the patches as solver problems on the device, the
    batched solve runs on those arrays in chunks of the handle's ``max_batch``, and k_probe_stamp writes the boolean maps
    k_path_plan reads (``qtos_path_plan*``, ``ShiftedWindows.repath(bool_map=...)``).  planner: a ``capi.Planner`` whose
    heightfields the caller has set as for ``feasibility_map`` -- ``heightfield.towr_map`` of the same maps, map m of the call
    being heightfield m of the handle.  maps_yx: n_maps x rows x cols or rows x cols, numpy or a tensor on the planner's device.
    stream: a torch stream (None: the current one).  The host reads one word in between, the number of problems.  Returns
    (bool_maps [n_maps, rows, cols] float64, offsets [n_maps + 1] int32, patch [N, 3] int32, status [N] int32), device tensors.
    An all-zero map yields no patch: the reference's check_flat_ground short-cut needs no special case."""
    import ctypes as C

    import torch

    from . import capi
    P, ptr, chk = planner, capi.ptr, planner._chk
    P._need("qtos_probe_device", "probe kernels")
    dev = torch.device("cuda", P.device)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    sp = C.c_void_p(stream.cuda_stream)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        maps = torch.as_tensor(maps_yx, **f64)
        maps = (maps[None] if maps.dim() == 2 else maps).contiguous()
        n_maps, rows, cols = maps.shape
        g = capi.probe_params(tuple(maps.shape), multi_map_shift, scale)
        offsets = torch.zeros((n_maps + 1,), **i32)
        slot = torch.zeros((n_maps, rows, max(cols // 2 - 1, 0)), **i32)
        cap = min(slot.numel(), 4096)                      # (room for a first call; a fleet with more patches calls again)
        while True:
            # (a word more than the capacity: an empty tensor has no device pointer)
            patch, start = torch.zeros((cap + 1, 3), **i32), torch.zeros((cap + 1, capi.START_DOUBLES), **f64)
            goal, map_id = torch.zeros((cap + 1, 3), **f64), torch.zeros((cap + 1,), **i32)
            chk(P.lib.qtos_probe_device(P.h, C.byref(g), ptr(maps), cap, ptr(offsets), ptr(slot), ptr(patch), ptr(start), ptr(goal),
                                        ptr(map_id), sp), "qtos_probe_device")
            N = int(offsets[-1].item())                    # the one word the host reads: the number of problems
            if N <= cap:
                break
            cap = N
        status = torch.full((N + 1,), -1, **i32)           # (every entry is written by the solve of its chunk)
        if N:
            nodes = torch.empty((min(N, P.max_batch), P.n), **f64)
            for c in range(0, N, P.max_batch):
                n = min(P.max_batch, N - c)
                chk(P.lib.qtos_plan_batch_device(P.h, n, ptr(start[c:]), ptr(goal[c:]), ptr(map_id[c:]), None, ptr(nodes), ptr(status[c:]),
                                                 None, None, sp), "qtos_plan_batch_device")
        bool_maps = torch.zeros((n_maps, rows, cols), **f64)
        chk(P.lib.qtos_probe_stamp_device(P.h, C.byref(g), ptr(offsets), ptr(slot), ptr(patch), ptr(status), ptr(bool_maps), sp),
            "qtos_probe_stamp_device")
    return bool_maps, offsets, patch[:N], status[:N]


def random_env_device(planner, base_yx, seeds, base_id=None, draws=None, n_shift=10, n_height=10, climb=False, delta=0.005, cell=None,
                      stream=None):
    """The reference's randomised terrains (``heightfield.random_env``) of n_maps windows without a host loop: k_terrain_env
    makes map m from base grid ``base_id[m]`` (None: base m) and the stream of ``random.seed(seeds[m])``, in both orientations,
    and the solver's one becomes the handle's terrain through ``set_heightfields_device`` -- map m of the call is heightfield m
    of the handle, as ``feasibility_maps_device`` expects.  planner: a ``capi.Planner``; base_yx: n_base x rows x cols or
    rows x cols, numpy or a tensor on the planner's device; seeds: n_maps ints (0 .. 2**63 - 1 as a tensor, 0 .. 2**64 - 1
    otherwise); draws: None, or an int32 device tensor [n_maps] of the outputs each stream has consumed, moved on in place
    (``n_shift=1, n_height=0`` on the current maps is the reference's ``update()``); cell: of the heightfields (None: 2 / rows,
    the reference's).  Returns (map_yx [n_maps, rows, cols] float64, status [n_maps] int32), device tensors; the heightfields
    are installed whatever the statuses are, and a map with a non-zero status is flat ground (``heightfield.random_env_table``
    names the statuses: 1 too many levels, 2 draws, 3 a NaN, 4 base_id)."""
    import ctypes as C

    import torch

    from . import capi
    P, ptr = planner, capi.ptr
    P._need("qtos_terrain_env_device", "terrain-env kernel")
    dev = torch.device("cuda", P.device)
    stream = torch.cuda.current_stream(dev) if stream is None else stream
    sp = C.c_void_p(stream.cuda_stream)
    f64, i32 = dict(dtype=torch.float64, device=dev), dict(dtype=torch.int32, device=dev)
    with torch.cuda.stream(stream):
        base = torch.as_tensor(base_yx, **f64)
        base = (base[None] if base.dim() == 2 else base).contiguous()
        if torch.is_tensor(seeds):
            seed = seeds.to(device=dev, dtype=torch.int64).contiguous()
        else:
            seed = torch.as_tensor(np.array([int(v) for v in np.ravel(seeds)], np.uint64).view(np.int64), device=dev)
        n_maps, (n_base, rows, cols) = seed.numel(), base.shape
        bid = None if base_id is None else torch.as_tensor(base_id, **i32).contiguous()
        if draws is not None and (not torch.is_tensor(draws) or draws.dtype != torch.int32 or draws.device != dev or draws.numel() != n_maps
                                  or not draws.is_contiguous()):
            raise ValueError("draws is a contiguous int32 tensor [n_maps] on the planner's device (it is moved on in place)")
        g = capi.terrain_env_params((n_base, rows, cols), n_maps, n_shift, n_height, climb, delta)
        map_yx, height_xy = torch.zeros((n_maps, rows, cols), **f64), torch.zeros((n_maps, cols, rows), **f64)
        status = torch.zeros((n_maps,), **i32)
        P._chk(P.lib.qtos_terrain_env_device(P.h, C.byref(g), ptr(base), ptr(bid), ptr(seed), ptr(draws), ptr(map_yx), ptr(height_xy),
                                             ptr(status), sp), "qtos_terrain_env_device")
        P.set_heightfields_device(height_xy, 2.0 / rows if cell is None else cell, stream=stream)
    return map_yx, status
