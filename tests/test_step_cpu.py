"""The interior-point restatement oracle/ipm.py on the CPU (no GPU): it is the C oracle's algorithm on every case of
step_cases.py and every prefix of the solve, the cases sit on the paths of k_step they are named for, and no Armijo decision
of any case is closer to its right-hand side than the margin under which test_gpu_steps.py would not decide it; the solves of
step_cases.STOPPED stop where qo_solve stops; a kappa_sigma <= 1 is refused.

The restatement's runs are shared through step_cases.run (one per problem and session)."""
import dataclasses

import numpy as np
import pytest

import step_cases as stc
from oracle import ipm
from oracle.oracle import oracle_options


@pytest.mark.parametrize("name", stc.QO_NAMES)
def test_restatement_is_the_oracles_algorithm_on_every_prefix(name):
    """ipm.solve(max_iter = k) against qo_solve(max_iter = k), k = 0 .. steps: iteration count, status, nodes to 1e-6 (the
    project's full-solve gate).  qo_solve does not look at the iterate its last iteration left: where the restatement finds
    that one converged, qo_solve says so with one more iteration allowed and takes no further step."""
    c = stc.case(name)
    worst = 0.0
    for b in range(c.B):
        R = stc.run(name, b)
        x0 = None if c.warm is None else c.warm[b]

        def oracle(k):
            return c.O.solve(c.q[b], x0=x0, opts=oracle_options(dataclasses.replace(c.cfg_full, max_iter=k), c.O))
        for k in range(c.steps + 1):
            kk = min(k, R["iters"])
            xo, info = oracle(k)
            err = float(np.abs(R["states"][kk]["x"] - xo).max())
            worst = max(worst, err)
            assert info.iters == kk, (name, b, k, info.iters, kk)
            assert err < stc.GATE_NODES, (name, b, k, err)
            converged = R["status"] == 0 and R["iters"] <= k
            if converged and R["iters"] == k:
                assert info.status == 1
                _, info = oracle(k + 1)
                assert info.iters == k
            assert info.status == (0 if converged else 1), (name, b, k, info.status)
    stc.record("cpu_restatement_vs_oracle", name, dict(problems=c.B, steps=c.steps, gate_nodes=stc.GATE_NODES, nodes=worst))


# what the restatement's run of a case has to show (any problem, any step)
EXPECT = {
    "two_base_polys": ("az<1", "chord", "latch", "mu_floor"),
    "short_last_poly": ("az<1",),
    "walk": ("amax<1", "az<1", "chord", "latch", "fresh_while_held", "mu_floor"),
    "trot": ("amax<1", "az<1", "chord", "mu_floor"),
    "knots100_trot": ("amax<1", "az<1", "chord", "two_chords"),
    "walk12": ("amax<1", "az<1"),
    "bilinear_1s": ("trials>1", "six_trials"),
    "bilinear_steps": ("amax<1", "trials>1", "six_trials"),
    "bilinear_no_qo": ("amax<1",),
    "hold": ("amax<1", "latch", "fresh_while_held"),
    "warm": ("warm_push",),
    "plain_mu": ("amax<1", "az<1", "no_chord"),
    "discard_small": ("rejected", "step_behind_rejected"),
    "discard_bilinear": ("rejected", "step_behind_rejected", "rejected_after_trials", "damped_behind_rejected"),
    "discard_trot": ("amax<1", "rejected", "step_behind_rejected", "rejected_after_trials"),
    "clip_small": ("clip", "clip_while_mu_moves"),
    "clip_trot": ("amax<1", "clip", "clip_while_mu_moves", "clip_registers_and_tail"),
}


def _shown(events):
    kinds = [e["kind"] for e in events]
    out = set()
    if any(e["amax"] < 1 for e in events):
        out.add("amax<1")
    if any(e["az"] < 1 and e["kind"] != 2 for e in events):
        out.add("az<1")
    if any(e["trials"] > 1 for e in events):
        out.add("trials>1")
    if any(e["trials"] == ipm.MAX_TRIALS and not e["log"][-1]["accepted"] for e in events):
        out.add("six_trials")
    if 1 in kinds:
        out.add("chord")
    if any(a == 1 and b == 1 for a, b in zip(kinds, kinds[1:])):
        out.add("two_chords")
    if 1 not in kinds and 2 not in kinds:
        out.add("no_chord")
    if 2 in kinds:
        out.add("rejected")
    if any(e["held"] for e in events):
        out.add("latch")
    if any(a["held"] and b["kind"] == 0 for a, b in zip(events, events[1:])):
        out.add("fresh_while_held")             # a factorisation with the hold weight in its diagonal
    if any(e["mu_floor"] for e in events):
        out.add("mu_floor")
    if any(len(e["clip_rows"]) for e in events):
        out.add("clip")
    for a, b in zip(events, events[1:]):
        if a["kind"] == 2:
            out.add("step_behind_rejected")           # the linearisation at x, not at the trial point; the chord ban
            assert b["kind"] == 0 and 1 not in [e["kind"] for e in events[events.index(a):]]
            if a["trials"] > 2:
                out.add("rejected_after_trials")
            if 0 < b["alpha"] < 1 and b["trials"] > 1:
                out.add("damped_behind_rejected")
    for e in events:
        # mu goes down behind a step longer than 0.3: there the limits at the old and at the new mu differ
        if len(e["clip_rows"]) and e["alpha"] > ipm.MU_STEP:
            out.add("clip_while_mu_moves")
            if (e["clip_rows"] < stc.KR * stc.ET).any() and (e["clip_rows"] >= stc.KR * stc.ET).any():
                out.add("clip_registers_and_tail")
    return out


def test_the_case_table_sits_on_the_paths_it_names():
    limit = stc.KR * stc.ET
    shown_by = {}
    for name in stc.NAMES:
        c = stc.case(name)
        runs = [stc.run(name, b) for b in range(c.B)]
        n_iq, n_eq = len(runs[0]["I"]), len(runs[0]["E"])
        assert n_iq == c.n_iq, (name, n_iq)
        shown = set().union(*[_shown(R["events"]) for R in runs])
        if c.warm is not None:
            # the warm start's slack push is the one that acts: a cold start from the same nodes would have other slacks
            R = runs[0]
            g0 = R["states"][0]["g"]
            s_warm, s_cold = (ipm.start_state(g0, R["lo"], R["hi"], R["row_kind"], c.cfg_full, w)[0] for w in (True, False))
            if np.array_equal(R["states"][0]["s"], s_warm[R["I"]]) and not np.array_equal(s_warm, s_cold):
                shown.add("warm_push")
        shown_by[name] = shown
        stc.record("cpu_case_table", name, dict(n_iq=n_iq, n_eqw=n_eq, shown=sorted(shown), iterations=[R["iters"] for R in runs],
                                                trials=[[e["trials"] for e in R["events"]] for R in runs]))
        missing = set(EXPECT[name]) - {"no_chord"} - shown
        assert not missing, (name, missing)
        if "no_chord" in EXPECT[name]:
            assert all("no_chord" in _shown(R["events"]) for R in runs), name
    rows = {n: (len(stc.run(n, 0)["I"]), len(stc.run(n, 0)["E"])) for n in stc.NAMES}
    assert rows["two_base_polys"][0] < stc.ET                                  # threads without a row
    assert stc.ET < rows["short_last_poly"][0] < limit                         # second register row half valid
    assert rows["walk"][0] == limit and rows["walk"][1] <= stc.KE * stc.ET     # exactly the register limit
    assert limit < rows["trot"][0] <= limit + stc.ET and rows["trot"][1] <= stc.KE * stc.ET      # a one-deep inequality tail only
    assert rows["knots100_trot"][1] > stc.KE * stc.ET                          # the equality tail
    assert rows["walk12"][0] > 2 * limit                                       # a tail three rows deep
    assert limit < rows["discard_trot"][0] and limit < rows["clip_trot"][0]     # the discarded step and the clip on tail rows
    # the paths that only settings reach are shown by the cases named for them and by no other (the product's settings do not
    # take them: step_cases.NOT_FOUND and the searches it records)
    assert stc.NOT_FOUND == ()
    assert [n for n in stc.NAMES if "rejected" in shown_by[n]] == stc.DISCARD_NAMES
    assert [n for n in stc.NAMES if "clip" in shown_by[n]] == stc.CLIP_NAMES
    # the stops: every STOPPED entry stops as the table says, in the iteration it says (None: it runs to convergence, which
    # the same solve with a jam counter that took the discarded step would not: alpha 1, 0, 0.25 -> jammed at 3)
    for entry in stc.STOPPED:
        name, b, _, stop, at = entry
        R = stc.run(name, b, stc.stopped_cfg(entry))
        assert R["stop"] == stop and (at is None or R["iters"] == at), (entry, R["stop"], R["iters"])
        al = [e["alpha"] for e in R["events"]]
        if stop == "jammed":
            sa = stc.stopped_cfg(entry).stall_alpha
            assert al[-1] < sa and al[-2] < sa and (len(al) == 2 or not al[-3] < sa)
        if stop == "converged":
            sa = stc.stopped_cfg(entry).stall_alpha
            k = [e["kind"] for e in R["events"]].index(2)
            assert al[k] == 0.0 and 0 < al[k + 1] < sa and al[k - 1] >= sa and R["status"] == 0


@pytest.mark.parametrize("name", stc.NAMES)
def test_no_armijo_decision_is_closer_than_the_exclusion_margin(name):
    """The condition that lets the GPU test exclude nothing: in the restatement's own run every trial's acceptance (the Armijo
    test, or the 1e-9 floor) stays what it is when the l1 infeasibility moves by the number of working rows times the gate on
    a constraint value."""
    c = stc.case(name)
    smallest = np.inf
    for b in range(c.B):
        R = stc.run(name, b)
        margin = stc.exclusion_margin(len(R["E"]) + len(R["I"]))
        for k, e in enumerate(R["events"]):
            for t, trial in enumerate(e["log"]):
                smallest = min(smallest, abs(trial["margin"]) / margin)
                assert stc.armijo_decision(trial["th"], trial["rhs"], margin) is trial["accepted"], (name, b, k, t, trial)
    stc.record("cpu_armijo_margins", name, dict(smallest_distance_from_the_armijo_rhs_over_exclusion_margin=float(smallest)))


def _stopped_id(entry):
    return "%s-%d-%s" % (entry[0], entry[1], entry[3])


@pytest.mark.parametrize("entry", stc.STOPPED, ids=_stopped_id)
def test_a_stopped_solve_stops_where_qo_solve_stops_and_hands_back_its_best_iterate(entry):
    """The stall rule, the jam rule and the best-iterate hand-back, which the cases (stall rules off) do not run, on the solves
    of step_cases.STOPPED: problem 1 of bilinear_steps under the product's settings (stall_iters = 5, stall_alpha = 1e-2,
    max_iter = 24) stalls in its ninth iteration; under stall_alpha = 0.9 three solves jam (two steps in a row shorter than
    that), one of them behind a long first step; and the two solves of discard_bilinear, whose discarded chord step (alpha 0)
    stands between a long step and a short one, must NOT jam.  The restatement stops where qo_solve stops, with its status, and
    both hand back the iterate with the lowest violation."""
    name, b, _, stop, at = entry
    c = stc.case(name)
    cfg = stc.stopped_cfg(entry)
    assert (cfg.stall_iters > 0 and cfg.stall_alpha > 0) if stop == "stalled" else cfg.stall_alpha > 0
    R = stc.run(name, b, cfg)
    assert R["stop"] == stop and R["status"] == (0 if stop == "converged" else 1) and R["iters"] < cfg.max_iter
    assert at is None or R["iters"] == at
    qo = name not in stc.NO_QO          # (the bilinear trot: qo_solve is no reference there, step_cases.NO_QO; the restatement alone)
    if qo:
        xo, info = c.O.solve(c.q[b], opts=oracle_options(cfg, c.O))
        assert (info.iters, info.status) == (R["iters"], R["status"])
    viols = [S["viol"] for S in R["states"]]
    best = int(np.argmin(viols))
    if stop == "stalled":
        assert R["iters"] - best >= cfg.stall_iters and best < R["iters"]
    if stop == "converged":
        best = R["iters"]
    assert np.array_equal(R["x"], R["states"][best]["x"])
    err = float(np.abs(R["x"] - xo).max()) if qo else None
    stc.record("cpu_stopped_solve", _stopped_id(entry), dict(problem=b, iterations=R["iters"], best_iterate=best, gate_nodes=stc.GATE_NODES, nodes=err,
                                                             alpha=[e["alpha"] for e in R["events"]]))
    assert not qo or err < stc.GATE_NODES
    # in front of the stop the stall rules change nothing: the events are those of the same settings without them
    off = stc.run(name, b, dataclasses.replace(stc.prefix(cfg), max_iter=R["iters"]))["events"]
    assert len(off) == R["iters"]
    for k in range(R["iters"]):
        assert (R["events"][k]["alpha"], R["events"][k]["trials"], R["events"][k]["kind"]) == (off[k]["alpha"], off[k]["trials"], off[k]["kind"])


def test_a_kappa_sigma_that_leaves_no_band_is_refused():
    """kappa_sigma <= 1 (or no number) is refused with a message where the configuration becomes the C structure, and by the
    library's own check of the parameters (what a C caller meets): the analysis fails; the default goes through."""
    import ctypes as C
    from qtos_amd import capi
    from qtos_amd.config import PlannerConfig
    assert PlannerConfig().kappa_sigma == ipm.KAPPA == 1e10
    for bad in (1.0, 0.5, 0.0, -3.0, float("nan")):
        with pytest.raises(ValueError, match="kappa_sigma must be > 1"):
            capi.params_from_config(PlannerConfig.reference_compat(kappa_sigma=bad))
    lib = capi.load()
    for value, rc in ((1e10, 0), (2.0, 0), (1.0, -1), (0.0, -1), (float("nan"), -1)):
        p = capi.params_from_config(PlannerConfig.reference_compat())
        p.kappa_sigma = value
        d = capi.QtosDims()
        assert lib.qtos_analyze(C.byref(p), C.byref(d), None, 0) == rc, value
