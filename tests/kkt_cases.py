"""Shared by test_kkt_cases_cpu.py and test_gpu_kkt_cases.py: one case per factor + solve kernel instantiation that a
transcription can select (kkt2_kernel, kkt3_kernel, kkt5_kernel and chord_kernel in csrc/qtos_planner.hip), the B = 3 problems
each case solves, the dense reference of those problems (LAPACK refined in extended precision on the oracle's Jacobian, cached
per transcription), the gates, the accuracy record.  No tests in here.

The front F of an instantiation decides at compile time (csrc/kkt2.hpp, kkt3.hpp, kkt5.hpp; branches(F) restates it):
  NT = F / 16 row tiles, NTILE = NT (NT + 1) / 2 Schur tiles on NU = kkt_pick_nu(NTILE) update waves, MAXT tiles per wave;
  NSV = 16 - NT service waves in phase AB; VP (F <= 128): U -= V P' from a fourth panel, else Y on the service waves;
  NBUF (F <= 128): two record buffers filled by LDS-DMA, else one through the prefetch registers; NH (NT <= 8): two waves
  per row tile in the backward pass, else one (Kkt2Cfg defines it; no kernel reads it today); HN = 15 - NT - (NT < 12) helper waves of the sweeps; NASM = 15 - 3 (NU >= 12)
  assembling waves; `true`: the code path of the continuation records.

The table is what scratch/kkt_census.py finds: per instantiation the smallest transcription (by n_unknowns) of the gaits as
they are -- the walk and the trot scaled to the horizon -- where one with at most 1000 unknowns reaches it, else the smallest
of the gaits cut to their first phases (`phases`: 1 = the robot stands, 3 = one step per foot) -- and of those the smallest on
which the reference and the method stay inside the gates on the host, without any kernel (test_kkt_cases_cpu.py):
  a reduced system only where the full system's step, the reference, is within half of GATE_REDUCED of what a system without
  the eliminated rows' multipliers gives (SEED_OF), else the smallest full system that reaches the instantiation;
  a full system only where a float64 block elimination in the planner's own order (order_floor: numpy, 16-pivot blocks inverted
  from their LDL' without pivoting, as the kernels eliminate) is within a fifth of the first-solve gate of the
  extended-precision step and keeps its panels below GATE_PANEL / eps_dual.  The transcriptions the census finds first for the fronts of 64, 96, 128, 160
  and 208 slots do not: on the walk of 0.3 s at 0.2 s knots, the walk of 0.75 s at 0.2 s knots and the transcriptions with
  dt_base = 0.5 .. 1 s over dt_dynamic = 0.05 .. 0.25 s the method itself loses the step to 1e-6 .. 6e-3 of its largest entry
  or grows panel entries of 2e9 (the kernels do the same there, measured on the MI355X: 1e-6 .. 3e-3), whatever the
  instantiation -- an elimination order for horizons and spacings no workload uses, on record in DESIGN.md section 5.  On
  the one-step walks and trots of 3 s at 0.05 s knots (96 .. 100 stages, fronts of 208 slots) the method's floor is 1e-6 .. 7e-5
  under barrier weights over six decades, at the gate itself: k_kkt2<208, true> measured 6e-6 .. 6e-5 there on the MI355X, as
  the host's elimination does (7e-6 .. 3e-5).
k_chord<F> of a case is the chord kernel of the same front: debug_chord and the refinement step run it.
"""
import json
import os
import re
import time

import numpy as np

from conftest import ROOT  # noqa: F401  (path set-up)

import spline_cases as sc
from oracle import ipm
from oracle.oracle import Oracle, oracle_dict
from oracle.oracle import lib as oracle_lib
from qtos_amd.config import REFERENCE_WALK_UNNORMALISED, TROT_UNNORMALISED, PlannerConfig, scaled_phases

B = 3
SEED = 7
NOISE = 0.01                               # on the starting point of the full-system cases
SIG_DECADES = (-3.0, 3.0)                  # barrier weights over six decades
GATE_FIRST = 5e-6                          # test_kkt_solve_matches_dense_reference: of the step's largest entry ...
GATE_CPU_SPREAD, GATE_SPREAD_FACTOR = 2.5e-7, 20.0   # ... where LAPACK and the oracle's LDL' agree to this, else 20 x their spread
GATE_REFINED = 1e-9                        # the same test: one refinement step against the extended-precision solution
GATE_REDUCED = 1e-7                        # test_reduced_base_system_gives_the_newton_step_of_the_full_system
GATE_CHORD = 1e-7                          # test_chord_step_kernel_matches_the_factorising_kernel
GATE_PANEL = 1.05                          # test_one_kkt_solve_is_accurate_on_every_transcription: |V| max x eps_dual
COND_UP_TO = 1000                          # unknowns of the full system up to which K's condition number is formed (an SVD)


def branches(F):
    """The compile-time constants of front F, as the kernels' headers define them."""
    NT = F // 16
    NTILE = NT * (NT + 1) // 2

    def pick_nu(ntile):
        if ntile == 21:
            return 12
        best, best_t = 14, (ntile + 13) // 14
        for nu in range(14, 7, -1):
            t = (ntile + nu - 1) // nu
            if t < best_t or (t == best_t and nu * t - ntile <= best * best_t - ntile):
                best, best_t = nu, t
        return max(ntile, 1) if ntile < 8 else best
    NU = pick_nu(NTILE)
    return dict(NT=NT, NTILE=NTILE, NU=NU, MAXT=(NTILE + NU - 1) // NU, NSV=16 - NT, VP=F <= 128, NBUF=2 if F <= 128 else 1,
                NH=2 if NT <= 8 else 1, HN=15 - NT - (1 if NT < 12 else 0), NASM=15 - (3 if NU >= 12 else 0))


def _t(gait, duration, dt_base, dt_dynamic=None, rom=0.08, force=1, reduced=True, phases=None):
    return dict(gait=gait, duration=duration, dt_base=dt_base, dt_dynamic=dt_base if dt_dynamic is None else dt_dynamic,
                dt_range_of_motion=rom, force_polys_per_stance=force, reduce_base=reduced, reduce_swing=reduced, phases=phases)


# The transcriptions of the table: (gait, duration, dt_base[, dt_dynamic], range-of-motion spacing, force polynomials per stance,
# the reduced system, phases per foot where the gait is cut)
TRANSCRIPTIONS = {
    "trot_0.5_0.5": _t("trot", 0.5, 0.5),
    "walk_0.5_0.5": _t("walk", 0.5, 0.5),
    "walk_0.3_0.25_full": _t("walk", 0.3, 0.25, reduced=False),
    "walk_0.5_0.25": _t("walk", 0.5, 0.25),
    "trot_stand_0.75_0.2_full": _t("trot", 0.75, 0.2, rom=0.2, reduced=False, phases=1),
    "trot_0.5_0.25_full": _t("trot", 0.5, 0.25, reduced=False),
    "trot_stand_0.5_0.05_full": _t("trot", 0.5, 0.05, reduced=False, phases=1),
    "stand_1_0.05": _t("walk", 1.0, 0.05, phases=1),
    "step_2_0.05_full": _t("walk", 2.0, 0.05, force=2, reduced=False, phases=3),
    "step_2.5_0.05_rom0.2_full": _t("walk", 2.5, 0.05, rom=0.2, force=2, reduced=False, phases=3),
    "step_2.5_0.05_full": _t("walk", 2.5, 0.05, force=2, reduced=False, phases=3),
    # (of the five one-step walks of 1577 unknowns that reach k_kkt2<208> the one with the method's floor furthest inside the gate;
    #  on the 3 s walk at 0.05 s knots and 0.08 s range-of-motion spacing it is 5e-6 of a gate of 2e-5: not admissible)
    "step_6_0.1_rom0.5_full": _t("walk", 6.0, 0.1, rom=0.5, force=2, reduced=False, phases=3),
    "trot_step_0.75_0.5": _t("trot", 0.75, 0.5, phases=3),
    "walk_2.5_0.1_dyn1": _t("walk", 2.5, 0.1, 1.0, force=3),
    "walk_2_0.25_full": _t("walk", 2.0, 0.25, reduced=False),
    "walk_0.75_0.5_full": _t("walk", 0.75, 0.5, reduced=False),
    "trot_1_0.5": _t("trot", 1.0, 0.5),
    "walk_2.5_1_full": _t("walk", 2.5, 1.0, reduced=False),
    "trot_1_0.5_full": _t("trot", 1.0, 0.5, reduced=False),
    "trot_2_1_full": _t("trot", 2.0, 1.0, reduced=False),
    "trot_2_1_rom0.2_full": _t("trot", 2.0, 1.0, rom=0.2, reduced=False),
    "trot_2.5_1_full": _t("trot", 2.5, 1.0, reduced=False),
    "trot_2.5_1_force2_full": _t("trot", 2.5, 1.0, force=2, reduced=False),
    # (smaller ones reach k_kkt2<208, true> too -- the standing robot of 2 .. 2.5 s at 0.05 s knots, 553 .. 1261 unknowns -- and are
    #  refused at planner creation, -4: stage records longer than the prefetch registers; the one-step walks and trots of 3 s at
    #  0.05 s knots, 1529 unknowns, are not admissible: the method's floor there is 1e-6 .. 7e-5 under every seed of 7 .. 19)
    "trot_step_5_0.1_force2_full": _t("trot", 5.0, 0.1, force=2, reduced=False, phases=3),
}

# name: (transcription, QTOS_KKT, the kernel kkt_kernel() names, n_unknowns, n_stages)
CASES = {
    # 32 slots: NT 2, 3 tiles on 3 update waves, 14 service waves, VP, two record buffers, NH 2, HN 12, NASM 15
    "kkt2_32": ("trot_0.5_0.5", "2", "k_kkt2<32>", 201, 13),
    "kkt3_32": ("trot_0.5_0.5", None, "k_kkt3<32, 1>", 201, 13),
    # 48 slots: NT 3, 6 tiles on 6 waves, 13 service waves, VP, NBUF 2, NH 2, HN 11, NASM 15
    "kkt2_48": ("walk_0.5_0.5", "2", "k_kkt2<48>", 141, 9),
    "kkt2_48_cont": ("trot_step_0.75_0.5", "2", "k_kkt2<48, true>", 105, 7),
    "kkt3_48": ("walk_0.5_0.5", None, "k_kkt3<48, 1>", 141, 9),
    # 64 slots: NT 4, 10 tiles on 10 waves, 12 service waves, VP, NBUF 2, NH 2, HN 10, NASM 15
    "kkt2_64": ("walk_0.3_0.25_full", "2", "k_kkt2<64>", 293, 19),
    "kkt2_64_cont": ("walk_2.5_0.1_dyn1", "2", "k_kkt2<64, true>", 561, 36),
    "kkt3_64": ("walk_0.3_0.25_full", None, "k_kkt3<64, 1>", 293, 19),
    # 80 slots: NT 5, 15 tiles on 8 waves (MAXT 2: the first front with two tiles on a wave), 11 service waves, VP, NBUF 2, NH 2, HN 9, NASM 15
    "kkt2_80": ("walk_0.5_0.25", "2", "k_kkt2<80>", 165, 11),
    "kkt2_80_cont": ("walk_2_0.25_full", "2", "k_kkt2<80, true>", 437, 28),
    "kkt3_80": ("walk_0.5_0.25", None, "k_kkt3<80, 1>", 165, 11),
    # 96 slots: NT 6, 21 tiles on 12 waves (kkt_pick_nu's exception), 10 service waves, VP, NBUF 2, NH 2, HN 8, NASM 12 (NU >= 12)
    "kkt2_96": ("trot_stand_0.75_0.2_full", "2", "k_kkt2<96>", 133, 9),
    "kkt2_96_cont": ("walk_0.75_0.5_full", "2", "k_kkt2<96, true>", 293, 19),
    "kkt3_96": ("trot_stand_0.75_0.2_full", None, "k_kkt3<96, 1>", 133, 9),
    "kkt5_96": ("walk_0.5_0.25", "6", "k_kkt5<96>", 165, 11),
    # 112 slots: NT 7, 28 tiles on 14 waves, 9 service waves (k_kkt3's waves 9 .. 15), VP, NBUF 2, NH 2, HN 7, NASM 12
    "kkt2_112": ("trot_0.5_0.25_full", "2", "k_kkt2<112>", 449, 29),
    "kkt2_112_cont": ("trot_1_0.5", "2", "k_kkt2<112, true>", 225, 15),
    "kkt3_112": ("trot_0.5_0.25_full", None, "k_kkt3<112, 1>", 449, 29),
    "kkt5_112": ("walk_0.75_0.5_full", "6", "k_kkt5<112>", 293, 19),
    # 128 slots: NT 8, 36 tiles on 12 waves (MAXT 3), 8 service waves, the last front with VP, NBUF 2 and NH 2; HN 6, NASM 12
    "kkt2_128": ("trot_stand_0.5_0.05_full", "2", "k_kkt2<128>", 277, 18),
    "kkt2_128_cont": ("walk_2.5_1_full", "2", "k_kkt2<128, true>", 317, 20),
    "kkt3_128": ("trot_stand_0.5_0.05_full", "4", "k_kkt3<128, 1>", 277, 18),
    "kkt5_128": ("trot_1_0.5", "6", "k_kkt5<128>", 225, 15),
    # 144 slots: NT 9, 45 tiles on 12 waves (MAXT 4), 7 service waves, the first front without VP (Y on the service waves),
    # with one record buffer through the prefetch registers and with NH 1; HN 5, NASM 12; k_kkt5: sweeps' helper waves off
    "kkt2_144": ("stand_1_0.05", "2", "k_kkt2<144>", 313, 20),
    "kkt2_144_cont": ("trot_1_0.5_full", "2", "k_kkt2<144, true>", 449, 29),
    "kkt5_144": ("trot_2_1_rom0.2_full", "6", "k_kkt5<144>", 449, 29),
    # 160 slots: NT 10, 55 tiles on 14 waves (MAXT 4), 6 service waves, no VP, NBUF 1, NH 1, HN 4, NASM 12
    "kkt2_160": ("step_2_0.05_full", "2", "k_kkt2<160>", 1097, 69),
    "kkt2_160_cont": ("trot_2_1_full", "2", "k_kkt2<160, true>", 449, 29),
    # 176 slots: NT 11, 66 tiles on 14 waves (MAXT 5), 5 service waves, no VP, NBUF 1, NH 1, HN 3 (the last NT < 12), NASM 12
    "kkt2_176": ("step_2.5_0.05_rom0.2_full", "2", "k_kkt2<176>", 1337, 85),
    "kkt2_176_cont": ("trot_2.5_1_full", "2", "k_kkt2<176, true>", 473, 30),
    # 192 slots: NT 12, 78 tiles on 13 waves (MAXT 6), 4 service waves, no VP, NBUF 1, NH 1, HN 3 (the first NT >= 12), NASM 12
    "kkt2_192": ("step_2.5_0.05_full", "2", "k_kkt2<192>", 1337, 84),
    "kkt2_192_cont": ("trot_2.5_1_force2_full", "2", "k_kkt2<192, true>", 665, 42),
    # 208 slots: NT 13, 91 tiles on 13 waves (MAXT 7), 3 service waves, no VP, NBUF 1, NH 1, HN 2, NASM 12; no idle helper waves
    # in the sweeps (the planner leaves sw_on off)
    "kkt2_208": ("step_6_0.1_rom0.5_full", "2", "k_kkt2<208>", 1577, 99),
    "kkt2_208_cont": ("trot_step_5_0.1_force2_full", "2", "k_kkt2<208, true>", 1337, 84),
}
NAMES = list(CASES)

# Compiled instantiations that no transcription of the census selects (scratch/kkt_census.py: both gaits, as they are and cut to
# 1, 3 and 5 phases per foot; horizons of 0.3 .. 20 s; dt_base and dt_dynamic of 0.05 .. 1 s, equal and unequal; three
# range-of-motion spacings; 1 .. 3 force polynomials per stance; the four combinations of the reduced systems; QTOS_KKT unset, 2,
# 4, 6).  Candidates for dead code; on record only.
_FRONT_16 = "no transcription of the census has a front below 32 slots"
UNREACHED = {
    "k_kkt2<16>": _FRONT_16,
    "k_kkt2<16, true>": _FRONT_16,
    "k_kkt3<16, 1>": _FRONT_16,
    "k_chord<16>": _FRONT_16,
    "k_kkt2<32, true>": "no transcription of the census with a front of 32 slots has continuation records",
}


def kernel_front(kernel):
    return int(re.match(r"k_\w+<(\d+)", kernel).group(1))


def chord_of(kernel):
    return "k_chord<%d>" % kernel_front(kernel)


def config(transcription):
    kw = dict(TRANSCRIPTIONS[transcription])
    n = kw.pop("phases")
    if n is not None:
        table = REFERENCE_WALK_UNNORMALISED if kw["gait"] == "walk" else TROT_UNNORMALISED
        kw["phase_durations"] = [scaled_phases([foot[:n]], kw["duration"])[0] for foot in table]   # (every foot's phases sum to T)
    return PlannerConfig(**kw)


class kkt_environment:
    """QTOS_KKT set (None: unset) and put back, as test_gpu_kernels.py's _planner does."""

    def __init__(self, kkt):
        self.kkt = kkt

    def __enter__(self):
        self.old = os.environ.get("QTOS_KKT")
        if self.kkt is None:
            os.environ.pop("QTOS_KKT", None)
        else:
            os.environ["QTOS_KKT"] = self.kkt

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("QTOS_KKT", None)
        else:
            os.environ["QTOS_KKT"] = self.old


def compiled_instantiations(text=None):
    """The instantiations of the product build, read out of the four selector functions of csrc/qtos_planner.hip as text: the
    branches of the development builds (QTOS_DEV_F128, QTOS_DEV_SMALL) are left out."""
    if text is None:
        text = open(os.path.join(ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc", "qtos_planner.hip")).read()

    def product_lines(body):
        """The lines a build without QTOS_DEV_F128 and QTOS_DEV_SMALL compiles."""
        keep, stack = [], []
        for line in body.splitlines():
            s = line.strip()
            if s.startswith("#if"):
                cond = s.split("//")[0]
                if s.startswith("#ifndef"):
                    on = True                                              # (#ifndef QTOS_DEV_...)
                elif s.startswith("#ifdef") or "!defined" not in cond:
                    on = False                                             # (#ifdef QTOS_DEV_...)
                else:
                    on = True                                              # (#if !defined(A) && !defined(B))
                stack.append(on)
            elif s.startswith("#else"):
                stack[-1] = not stack[-1]
            elif s.startswith("#endif"):
                stack.pop()
            elif all(stack) and not s.startswith("#define"):
                keep.append(line)
        assert not stack
        return "\n".join(keep)

    out = set()
    for fn, macro, names in (("kkt2_kernel", "QTOS_KKT2", ("k_kkt2<%d>", "k_kkt2<%d, true>")), ("kkt3_kernel", "QTOS_KKT3", ("k_kkt3<%d, 1>",)),
                             ("kkt5_kernel", "QTOS_KKT5", ("k_kkt5<%d>",)), ("chord_kernel", "QTOS_CHORD", ("k_chord<%d>",))):
        m = re.search(r"^static void \(\*%s\(.*?^}" % fn, text, re.S | re.M)
        assert m, fn
        fronts = [int(f) for f in re.findall(r"%s\((\d+)\)" % macro, product_lines(m.group(0)))]
        assert fronts and len(set(fronts)) == len(fronts), (fn, fronts)
        out |= {n % f for f in fronts for n in names}
    return out


def table_instantiations():
    """The factor kernel of every case and the k_chord of its front."""
    return {CASES[n][2] for n in NAMES} | {chord_of(CASES[n][2]) for n in NAMES}


# Seeds other than SEED.  stand_1_0.05: under seeds 7 .. 11 LAPACK and the oracle's LDL' are 2.9e-7 .. 4.9e-7 of the step apart on
# one of the three problems (LAPACK is 1e-12 from the extended-precision solution: the spread is the oracle's), which would
# widen the first-solve gate; under 12 they agree to 2.4e-7 on all three.  The `step_*` transcriptions have a spread of
# 1e-7 .. 1.4e-6 under every seed tried (7 .. 12): their first-solve gate is 20 x the spread, 3e-5 of the step at most.
# The reduced transcriptions: the seed is the first of 7, 8, ... under which the full system's step -- the reference -- is within
# half of GATE_REDUCED of the step with (almost) no regularisation on the eliminated rows' multipliers (floor "reduced_vs_full";
# 1.1e-7 .. 1.4e-7 under seed 7 on the three named after stand_1_0.05).  Where no seed of 7 .. 15 gives that (barrier weights over
# six decades: 5e-8 .. 3e-6 on the walks of 0.75 s / 0.2 s, 1 s / 0.5 s / 0.05 s, 0.5 s / 0.2 s, 1 s / 0.5 s and the trot of
# 2.5 s / 1 s) the table has the smallest full system that reaches the instantiation instead.
SEED_OF = {"stand_1_0.05": 12, "walk_0.5_0.25": 10, "trot_step_0.75_0.5": 8, "trot_1_0.5": 13}

# ---- the problems of a case and their dense reference ---------------------------------------------------------------
_refs = {}


class Reference:
    pass


def reference(transcription, seed=None):
    """The B problems of a transcription and the dense solution of each, built once and shared by the cases on it.

    Full system (reduce_base and reduce_swing off): x = the oracle's starting point + NOISE N(0, 1), the fixed variables on
    their bounds.  Reduced system: the starting point itself, the swing mid nodes on the swing rule -- a point of both spaces,
    at which the step of the reduced system is the step of the full one (GATE_REDUCED).  sig over SIG_DECADES and w ~ N(0, 1)
    on the inequality rows, everything from the transcription's seed; the three problems have their own start, goal, x, sig and w.
    The reference of a problem is ipm.solve_refined on ipm.kkt_matrix / kkt_rhs of the oracle's Jacobian and constraint values
    (the largest full system of the table has 1577 unknowns: every K is formed)."""
    if seed is None:
        if transcription in _refs:
            return _refs[transcription]
        seed = SEED_OF.get(transcription, SEED)
    t0 = time.time()
    R = Reference()
    R.transcription = transcription
    R.cfg = cfg = config(transcription)
    R.reduced = bool(cfg.reduce_base or cfg.reduce_swing)
    R.O = O = Oracle(oracle_dict(cfg))
    rng = np.random.default_rng(seed)
    start, goal = sc.problems(B, seed)
    goal[:, 0] = start[:, 0] + (goal[:, 0] - start[:, 0]) * (cfg.duration / 5.0)       # (the walking speed of the 5 s plans)
    R.start, R.goal = start, goal
    R.q = [sc.oracle_problem(O, cfg, start[b], goal[b]) for b in range(B)]
    R.free, R.E, R.I, R.lo, R.hi, R.row_kind = ipm.working_set(O, R.q[0])
    lo, hi = O.var_bounds(R.q[0])
    R.fixed = lo == hi
    x = np.stack([O.start_point(q) for q in R.q])
    if not R.reduced:
        x = x + NOISE * rng.standard_normal(x.shape)
    for b, q in enumerate(R.q):
        lo, hi = O.var_bounds(q)
        assert np.array_equal(lo == hi, R.fixed)
        x[b, R.fixed] = lo[R.fixed]
    R.x = x
    R.sig, R.w = np.zeros((B, O.m)), np.zeros((B, O.m))
    R.sig[:, R.I] = 10.0 ** rng.uniform(SIG_DECADES[0], SIG_DECADES[1], (B, len(R.I)))
    R.w[:, R.I] = rng.standard_normal((B, len(R.I)))
    R.nf, R.nE = len(R.free), len(R.E)
    R.J = [O.jacobian(x[b]) for b in range(B)]
    R.g = [O.constraints(x[b]) for b in range(B)]
    R.problems = [_dense(R, b) for b in range(B)]
    R.cond, R.order_floor = {}, {}
    R.seconds = time.time() - t0
    if seed == SEED_OF.get(transcription, SEED):
        _refs[transcription] = R
    return R


def _dense(R, b):
    """Problem b: the extended-precision step, LAPACK's own, the oracle's LDL', the first-solve gate and the reference's floor."""
    import ctypes as C
    cfg, nf = R.cfg, R.nf
    K = ipm.kkt_matrix(R.J[b], R.free, R.E, R.I, R.sig[b], cfg.delta_x, np.full(R.nE, cfg.eps_dual))
    rhs = ipm.kkt_rhs(R.J[b], R.g[b], R.free, R.E, R.I, R.w[b])
    hp, corr, lu = ipm.solve_refined(K, rhs)
    from scipy.linalg import lu_solve
    lapack = lu_solve(lu, rhs)[:nf]
    P = Reference()
    P.step = hp[:nf].astype(np.float64)
    P.scale = float(np.abs(P.step).max())
    P.lapack = lapack
    sol = rhs.copy()
    Kc = np.ascontiguousarray(K)
    dp = C.POINTER(C.c_double)
    assert oracle_lib().qo_ldlt_solve_dense(nf + R.nE, Kc.ctypes.data_as(dp), sol.ctypes.data_as(dp)) == 0
    P.oracle = sol[:nf]
    P.cpu_spread = float(np.abs(P.oracle - lapack).max())
    P.gate_first = GATE_FIRST * P.scale if P.cpu_spread < GATE_CPU_SPREAD * P.scale else GATE_SPREAD_FACTOR * P.cpu_spread
    P.floor = dict(lapack_vs_extended=float(np.abs(lapack - P.step).max() / P.scale), lapack_vs_oracle=P.cpu_spread / P.scale,
                   last_correction=float(np.abs(corr[:nf]).max() / P.scale))
    if R.reduced:
        # what the full system's eps_dual on the eliminated rows' multipliers moves the step by: the distance a reduced system,
        # which has no such multipliers, keeps from this reference however well it is solved
        eps = np.where(eliminated_rows(R)[R.E], 1e-13, cfg.eps_dual)
        h13, _, _ = ipm.solve_refined(ipm.kkt_matrix(R.J[b], R.free, R.E, R.I, R.sig[b], cfg.delta_x, eps), rhs)
        P.floor["reduced_vs_full"] = float(np.abs(h13[:nf].astype(np.float64) - P.step).max() / P.scale)
    return P


def eliminated_rows(R):
    """Mask of the rows whose multipliers a reduced system does not have: the base's acceleration continuity (reduce_base) and
    the swing rule (reduce_swing, nearest-cell terrain), by the oracle's layout."""
    cfg, L, r = R.cfg, R.O.L, np.arange(R.O.m)
    out = np.zeros(R.O.m, bool)
    if cfg.reduce_base:
        out |= (r >= L.off_acc_lin) & (r < L.off_rom[0])
    if cfg.reduce_swing and cfg.terrain_mode == 1:
        out |= r >= L.off_swing[0]
    return out


def _inverse_unpivoted(Bk):
    """(L D L')^-1 = L^-T D^-1 L^-1 of a pivot block from its LDL' without pivoting, the pivots in the order they have in the
    block, the block read from its lower triangle: what wave 0 of the kernels forms (kkt2_factor_block, ldlt16s)."""
    from scipy.linalg import solve_triangular
    n = len(Bk)
    T, L, D = np.tril(Bk) + np.tril(Bk, -1).T, np.eye(n), np.zeros(n)
    for j in range(n):
        D[j] = T[j, j]
        L[j + 1:, j] = T[j + 1:, j] / D[j]
        T[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], T[j + 1:, j])
    Linv = solve_triangular(L, np.eye(n), lower=True, unit_diagonal=True)
    return Linv.T @ (Linv / D[:, None])


def order_floor(R, b):
    """What float64 leaves of problem b's step when K is eliminated as the kernels eliminate it, in plain numpy: in the
    planner's order (capi.analyze_order: no GPU), 16 pivots at a time, every pivot block inverted explicitly from its LDL'
    without any pivoting, V = P B^-1, the Schur complement kept exactly symmetric (its lower triangle is what is stored).
    Returns (max |step - extended-precision step| / scale, the largest entry of the factor panels V): the floor of the METHOD
    on this transcription and these barrier weights, whatever kernel runs it -- an estimate, since the order of the sums is
    not the kernels' (on the MI355X the kernels are between 0.1 and 3 times this away).  Full systems only (the order of a
    reduced system is over unknowns the oracle does not have): (None, None) for a reduced one."""
    if R.reduced:
        return None, None
    if b not in R.order_floor:
        from qtos_amd import capi
        with kkt_environment(None):
            order = capi.analyze_order(R.cfg)
        pos_of = {int(v): i for i, v in enumerate(R.free)}
        pos_of.update({R.O.n + int(r): R.nf + i for i, r in enumerate(R.E)})
        stages = [[pos_of[int(u)] for u in order[k:k + 16] if u >= 0] for k in range(0, len(order), 16)]
        perm = np.array([i for st in stages for i in st])
        assert np.array_equal(np.sort(perm), np.arange(R.nf + R.nE))
        cfg = R.cfg
        K = ipm.kkt_matrix(R.J[b], R.free, R.E, R.I, R.sig[b], cfg.delta_x, np.full(R.nE, cfg.eps_dual))
        A = K[np.ix_(perm, perm)]
        y = ipm.kkt_rhs(R.J[b], R.g[b], R.free, R.E, R.I, R.w[b])[perm]
        kept, o, vmax = [], 0, 0.0
        for st in stages:
            e = o + len(st)
            Binv = _inverse_unpivoted(A[o:e, o:e])
            rows = e + np.flatnonzero(np.abs(A[e:, o:e]).max(axis=1) > 0) if e < len(A) else np.zeros(0, int)   # the front
            P = A[rows, o:e]
            V = P @ Binv
            vmax = max(vmax, float(np.abs(V).max()) if V.size else 0.0)
            S = A[np.ix_(rows, rows)] - V @ P.T
            A[np.ix_(rows, rows)] = np.tril(S) + np.tril(S, -1).T
            y[rows] -= V @ y[o:e]
            kept.append((o, e, rows, V, Binv))
            o = e
        x = np.zeros_like(y)
        for o, e, rows, V, Binv in reversed(kept):
            x[o:e] = Binv @ y[o:e] - V.T @ x[rows]
        h = np.empty_like(x)
        h[perm] = x
        R.order_floor[b] = (float(np.abs(h[:R.nf] - R.problems[b].step).max() / R.problems[b].scale), vmax)
    return R.order_floor[b]


def condition(R, b):
    """cond(K) of problem b (an SVD: for the record, not formed with the reference), None above COND_UP_TO unknowns."""
    if R.nf + R.nE > COND_UP_TO:
        return None
    if b not in R.cond:
        R.cond[b] = float(np.linalg.cond(ipm.kkt_matrix(R.J[b], R.free, R.E, R.I, R.sig[b], R.cfg.delta_x, np.full(R.nE, R.cfg.eps_dual))))
    return R.cond[b]


def record(section, name, entry):
    """Print a check's figures; where the environment variable QTOS_KKT_ACCURACY names a file, keep them in it as JSON
    (profiles/kkt_instantiation_accuracy.json is such a file from an MI355X run)."""
    print("kkt accuracy [%s, %s]: %s" % (section, name, json.dumps(entry)))
    path = os.environ.get("QTOS_KKT_ACCURACY")
    if path:
        data = json.load(open(path)) if os.path.exists(path) else {}
        data.setdefault(section, {})[name] = entry
        json.dump(data, open(path, "w"), indent=1, sort_keys=True)
