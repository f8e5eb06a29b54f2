"""Which transcription reaches which factor + solve kernel instantiation (no GPU: capi.analyze_kernel / capi.analyze).

    python scratch/kkt_census.py [out.json] [stage ...]

For every compiled instantiation the smallest transcription (by n_unknowns) of the grid below that selects it, under QTOS_KKT
unset, 2, 4 and 6.  tests/kkt_cases.py is made from this list; an instantiation that no transcription reaches goes into its
UNREACHED.  Stages (default: all): `equal` (dt_base = dt_dynamic over every duration), `unequal` (dt_base != dt_dynamic on the
short horizons), `phases` (gaits cut to their first phases, a standing robot), `long` (the long horizons without continuation
records: other range-of-motion spacings and force polynomials).
"""
import itertools
import json
import multiprocessing
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KKT = (None, "2", "4", "6")
REDUCE = ((True, True), (False, False), (True, False), (False, True))
DURATIONS = (0.3, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0, 4.0, 5.0, 6.0, 8.0, 10.0, 12.0, 16.0, 20.0)
DTS = (0.05, 0.1, 0.2, 0.25, 0.5, 1.0)
ROMS = (0.08, 0.2, 0.5)
FORCE = (1, 2, 3)


def grid(stages):
    out = []
    if "equal" in stages:
        for gait, dur, dt, rom, fp, red in itertools.product(("walk", "trot"), DURATIONS, DTS, ROMS, FORCE, REDUCE):
            if dt <= dur and dur / dt <= 240:
                out.append(dict(gait=gait, duration=dur, dt_base=dt, dt_dynamic=dt, dt_range_of_motion=rom, force_polys_per_stance=fp,
                                reduce_base=red[0], reduce_swing=red[1]))
    if "unequal" in stages:
        for gait, dur, db, dd, rom, red in itertools.product(("walk", "trot"), DURATIONS[:8], DTS, DTS, ROMS[::2], REDUCE[:2]):
            if db != dd and max(db, dd) <= dur and dur / min(db, dd) <= 120:
                out.append(dict(gait=gait, duration=dur, dt_base=db, dt_dynamic=dd, dt_range_of_motion=rom, reduce_base=red[0], reduce_swing=red[1]))
    if "phases" in stages:
        for gait, n, dur, dt, rom, fp, red in itertools.product(("walk", "trot"), (1, 3, 5), DURATIONS[:8], DTS, ROMS, FORCE, REDUCE[:2]):
            if dt <= dur:
                out.append(dict(gait=gait, phases=n, duration=dur, dt_base=dt, dt_dynamic=dt, dt_range_of_motion=rom, force_polys_per_stance=fp,
                                reduce_base=red[0], reduce_swing=red[1]))
    if "long" in stages:
        for gait, dur, dt, rom, fp, red in itertools.product(("walk", "trot"), DURATIONS[8:], DTS[:4], (0.04, 0.08, 0.2, 0.5, 1.0), (1, 2, 3, 4, 6), REDUCE[:2]):
            if dur / dt <= 400:
                out.append(dict(gait=gait, duration=dur, dt_base=dt, dt_dynamic=dt, dt_range_of_motion=rom, force_polys_per_stance=fp,
                                reduce_base=red[0], reduce_swing=red[1]))
    return out


def config(point):
    from qtos_amd.config import REFERENCE_WALK_UNNORMALISED, TROT_UNNORMALISED, PlannerConfig, scaled_phases
    kw = dict(point)
    n = kw.pop("phases", None)
    if n is not None:
        table = REFERENCE_WALK_UNNORMALISED if kw["gait"] == "walk" else TROT_UNNORMALISED
        kw["phase_durations"] = [scaled_phases([foot[:n]], kw["duration"])[0] for foot in table]   # (every foot's phases sum to T)
    return PlannerConfig(**kw)


def visit(point):
    """[(kernel, QTOS_KKT, n_unknowns, n_stages, front of the default analysis)] of one grid point, one entry per QTOS_KKT."""
    from qtos_amd import capi
    out = []
    try:
        cfg = config(point)
        os.environ.pop("QTOS_KKT", None)
        d, _ = capi.analyze(cfg)
    except Exception:
        return point, out
    for kkt in KKT:
        if kkt is None:
            os.environ.pop("QTOS_KKT", None)
        else:
            os.environ["QTOS_KKT"] = kkt
        try:
            out.append((capi.analyze_kernel(cfg), kkt, int(d.n_unknowns), int(d.n_stages), int(d.front)))
        except Exception:
            pass
    os.environ.pop("QTOS_KKT", None)
    return point, out


def main():
    args = sys.argv[1:]
    path = args[0] if args and args[0].endswith(".json") else None
    stages = [a for a in args if not a.endswith(".json")] or ["equal", "unequal", "phases", "long"]
    points = grid(stages)
    print("%d transcriptions x %d choices of QTOS_KKT" % (len(points), len(KKT)), flush=True)
    best, fronts = {}, {}
    null = os.open(os.devnull, os.O_WRONLY)
    os.dup2(null, 2)                      # (the analysis says on stderr why a transcription is refused)
    with multiprocessing.Pool(min(16, os.cpu_count() or 1)) as pool:
        for point, found in pool.imap_unordered(visit, points, chunksize=16):
            for kernel, kkt, n, stages_, front in found:
                fronts[front] = fronts.get(front, 0) + 1
                if kernel not in best or (n, str(kkt)) < (best[kernel]["n_unknowns"], str(best[kernel]["kkt"])):
                    best[kernel] = dict(n_unknowns=n, n_stages=stages_, kkt=kkt, point=point)
    for k in sorted(best, key=lambda k: (k.split("<")[0], int(k.split("<")[1].split(",")[0].rstrip(">")), k)):
        print("%-18s %5d unknowns %4d stages  QTOS_KKT=%s  %s" % (k, best[k]["n_unknowns"], best[k]["n_stages"], best[k]["kkt"], json.dumps(best[k]["point"])))
    print("%d instantiations reached; fronts of the default analysis seen: %s" % (len(best), sorted(fronts)))
    if path:
        json.dump(best, open(path, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
