#!/usr/bin/env python3
"""Generate tests/golden/random_env.json from the reference's own terrain randomiser.

Runs where make_golden.py runs (it imports the reference the same way); the test-suite reads the committed output only.
`Height_Map_Generator.__init__(randomize_env=True)` (QTOS/generateHeightField.py:563-567) and `update()` (:584-588) run as they
are, on python's module-level `random` stream, in a scratch directory that holds a copy of the reference's tile files (the
constructor writes its two height files next to them).  A spy in place of the module's `random` records what every draw
returned: the net shift of a case and the merge case's dry run are read off that record.  No reference source text is
copied: only data.
"""
import hashlib
import json
import os
import random
import shutil
import sys
import tempfile
import types

import numpy as np

from make_golden import OUT, REF

TILE_SETS = (
    ("exp_1", ["plane", "plane"], (1,)),
    ("exp_3", ["feasibility", "feasibility_1", "plane"], (1, 2)),
    ("exp_5", ["climb_2", "climb_1"], (1,)),
)
SEEDS = (0, 1, 2, 7, 12345, 2**32 + 5)
STEP = {"left": (0, -1), "right": (0, 1), "up": (-1, 0), "down": (1, 0)}


class Spy:
    """The `random` module as generateHeightField sees it: every call goes to the real stream, and is recorded."""

    def __init__(self):
        self.log = []

    def choice(self, seq):
        v = random.choice(seq)
        self.log.append(("choice", v))
        return v

    def uniform(self, a, b):
        v = random.uniform(a, b)
        self.log.append(("uniform", v))
        return v


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype="<f8").tobytes()).hexdigest()


def levels(a):
    a = np.asarray(a)
    return [float(v) for v in np.unique(a[a != 0])]


def net_shift(log, n_shift):
    """(dy, dx) of the map: the second run of n_shift direction draws (the first moves the solver copy)."""
    picks = [v for k, v in log if k == "choice" and isinstance(v, str)]
    assert len(picks) >= 2 * n_shift
    dy = sum(STEP[d][0] for d in picks[n_shift:2 * n_shift])
    dx = sum(STEP[d][1] for d in picks[n_shift:2 * n_shift])
    return [dy, dx]


def main():
    sys.modules.setdefault("pybullet", types.ModuleType("pybullet"))
    sys.path.insert(0, REF)
    cwd = os.getcwd()
    tmp = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(tmp, "data"))
        shutil.copytree(os.path.join(REF, "data", "heightfields"), os.path.join(tmp, "data", "heightfields"))
        os.makedirs(os.path.join(tmp, "data", "heightfields", "from_pybullet"), exist_ok=True)
        os.chdir(tmp)
        from QTOS import generateHeightField as ghf
        spy = Spy()
        ghf.random = spy
        out = {"seeds": list(SEEDS), "n_height": 10, "delta": 0.005, "bases": {}, "cases": []}
        for name, tiles, scales in TILE_SETS:
            base1 = np.array(ghf.Maps(tiles, 20, 1).map, dtype=float)
            climb = bool(ghf.Height_Map_Generator.climb_map_check(None, tiles))
            out["bases"][name] = {"tiles": tiles, "climb": climb, "map": base1.tolist()}
            for scale in scales:
                base = np.array(ghf.Maps(tiles, 20, scale).map, dtype=float)
                assert np.array_equal(base, np.repeat(np.repeat(base1, scale, axis=0), scale, axis=1))
                for seed in SEEDS:
                    spy.log = []
                    random.seed(seed)
                    g = ghf.Height_Map_Generator(maps=tiles, scale_factor=scale, randomize_env=True)
                    nxt = random.getrandbits(32)
                    m = np.array(g.map, dtype=float)
                    assert g.climb_map == climb and m.shape == base.shape
                    case = {"base": name, "mesh_scale": scale, "seed": seed, "n_shift": 10 * scale, "climb": climb,
                            "net_shift": net_shift(spy.log, 10 * scale), "levels": levels(m), "sha256": sha(m),
                            "next_bits": nxt, "n_calls": len(spy.log)}
                    if scale == 1 and m.any():              # (a map of zeros is its sha256 and its shape)
                        case["map"] = m.tolist()
                    out["cases"].append(case)
        # update(): two calls behind a constructor's sequence
        tiles = TILE_SETS[1][1]
        random.seed(7)
        g = ghf.Height_Map_Generator(maps=tiles, scale_factor=1, randomize_env=True)
        steps = []
        for _ in range(2):
            g.update()
            steps.append({"map": np.array(g.map, dtype=float).tolist()})
        out["update"] = {"base": "exp_3", "seed": 7, "n_shift": 10, "steps": steps, "next_bits": random.getrandbits(32)}
        # random_map_shift alone
        base = np.array(out["bases"]["exp_3"]["map"])
        out["map_shift"] = []
        for seed, shift, climb in ((3, 1, False), (4, 25, False), (5, 25, True)):
            obj = object.__new__(ghf.Height_Map_Generator)
            obj.climb_map = climb
            random.seed(seed)
            m = obj.random_map_shift(base.copy(), shift)
            out["map_shift"].append({"base": "exp_3", "seed": seed, "shift": shift, "climb": climb, "map": np.asarray(m).tolist(),
                                     "next_bits": random.getrandbits(32)})
        # the merge case: two levels, the second where the first lands in the map's first pass
        obj = object.__new__(ghf.Height_Map_Generator)
        obj.climb_map = False
        h1, far = 0.05, 0.2
        two = np.zeros((6, 8))
        two[1:3, 2:5], two[4, 5:7] = h1, far

        def run(m, seed):
            spy.log = []
            random.seed(seed)
            obj.towr_map = np.transpose(m)
            t = obj.random_height_shift(obj.random_map_shift(obj.towr_map, 0), 10)
            n_towr = len(spy.log)
            r = obj.random_height_shift(obj.random_map_shift(m, 0), 10)
            return np.asarray(r, dtype=float), spy.log[n_towr:], len(spy.log), random.getrandbits(32), np.asarray(t)
        for seed in range(100):
            _, log, _, _, _ = run(two, seed)
            d, c = log[0][1], log[1][1]                    # what the map's first pass applies to h1
            h2 = h1 + d if c == 0 else h1 - d
            if c != 2 and h1 < h2 < far:                   # (h1 stays the first level of the pass)
                break
        merged = two.copy()
        merged[4, 5:7] = h2
        m_sep, _, calls_sep, next_sep, _ = run(two, seed)
        m_mrg, _, calls_mrg, next_mrg, _ = run(merged, seed)
        assert len(levels(m_mrg)) == 1 and calls_mrg < calls_sep
        out["merge"] = {"seed": seed, "h1": h1, "h2": float(h2), "d": float(d), "choice": int(c),
                        "separate": {"base": two.tolist(), "map": m_sep.tolist(), "n_calls": calls_sep, "next_bits": next_sep},
                        "merged": {"base": merged.tolist(), "map": m_mrg.tolist(), "n_calls": calls_mrg, "next_bits": next_mrg}}
    finally:
        os.chdir(cwd)
        shutil.rmtree(tmp, ignore_errors=True)
    with open(os.path.join(OUT, "random_env.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
    print("random_env.json: %d cases, %d bytes" % (len(out["cases"]), os.path.getsize(os.path.join(OUT, "random_env.json"))))


if __name__ == "__main__":
    sys.exit(main())
