"""Every factor + solve kernel instantiation a transcription can select (tests/kkt_cases.py: 34 of k_kkt2, k_kkt3 and k_kkt5,
with the k_chord of the same front) against a dense solve of the same system on the host: LAPACK refined with residuals in
extended precision on the oracle's Jacobian and constraint values (oracle/ipm.py).  No kernel of the project judges here.

Per case one planner of three problems under the case's QTOS_KKT and four launches: debug_newton, debug_chord,
debug_residual(refine) and the factor panels.  The gates are the project's (kkt_cases.GATE_*):
  first solve and chord step   5e-6 of the step's largest entry where LAPACK and the oracle's LDL' agree to 2.5e-7 of it, else
                               20 x their spread (test_kkt_solve_matches_dense_reference)
  one refinement step          1e-9 against the extended-precision solution; a reduced system 1e-7 against the step of the full
                               system at a point of both spaces (test_reduced_base_system_gives_the_newton_step_of_the_full_system)
  chord against the first      1e-7 of the first solve's largest entry (test_chord_step_kernel_matches_the_factorising_kernel)
  factor panels                no entry above 1.05 / eps_dual (test_one_kkt_solve_is_accurate_on_every_transcription)
  fixed variables              a step of exactly 0
The host reference of the slowest transcription (1577 unknowns) takes 2 s, all 24 transcriptions together 20 s: most of the
file's time next to the MI355X.
All 34 cases pass there (profiles/kkt_instantiation_accuracy.json); no case is refused for the LDS.
"""
import numpy as np
import pytest

import kkt_cases as kc

pytestmark = pytest.mark.gpu

_refused = []       # cases whose planner the library refused for the LDS (-4): one at most, named in the output


@pytest.mark.parametrize("name", kc.NAMES)
def test_instantiation_matches_the_dense_solve(name):
    from qtos_amd.capi import Planner
    from test_gpu_selftest import _is_lds_refusal
    transcription, kkt, kernel, unknowns, stages = kc.CASES[name]
    R = kc.reference(transcription)
    cfg, B = R.cfg, kc.B
    with kc.kkt_environment(kkt):
        try:
            P = Planner(cfg, max_batch=B)
        except RuntimeError as exc:
            if not _is_lds_refusal(exc):
                raise
            _refused.append(name)
            print("[kkt cases] planner refused for the LDS (-4): %s" % _refused)
            assert len(_refused) <= 1, _refused
            pytest.skip("the library refuses %s for the LDS (-4)" % name)
    try:
        assert P.kkt_kernel() == kernel, P.kkt_kernel()
        assert P.dims.n_unknowns == unknowns
        assert kernel.startswith("k_kkt5") or P.dims.n_stages == stages      # (the pair-mode analysis has its own stages)
        assert (P.n, P.m) == (R.O.n, R.O.m)
        rk, vf, _ = P.structure()
        # the working set is the one the reference was built on
        assert np.array_equal(np.nonzero(vf != 0)[0], R.free) and np.array_equal(np.nonzero(rk == 2)[0], R.I)
        if R.reduced:
            assert set(np.nonzero(rk == 1)[0]) <= set(R.E) and kc.eliminated_rows(R)[R.E[rk[R.E] != 1]].all()
        else:
            assert np.array_equal(np.nonzero(rk == 1)[0], R.E)
        try:
            dx = P.debug_newton(R.start, R.goal, R.x, R.sig, R.w)
            dc = P.debug_chord(B)
            dr, _ = P.debug_residual(B, refine=True)
            vmax = max(float(np.abs(P.factor(b)[0][:, 1:, :]).max()) for b in range(B))
        except RuntimeError as exc:     # a HIP error: nothing this process starts on the GPU after it means anything
            pytest.exit("HIP error in case %s (%s): %s" % (name, kernel, exc), returncode=3)
    finally:
        P.close()
    free, fixed = R.free, R.fixed
    entry = dict(kernel=kernel, chord=kc.chord_of(kernel), front=kc.kernel_front(kernel), stages=stages, unknowns=unknowns,
                 transcription=transcription, reduced=R.reduced, full_system_unknowns=R.nf + R.nE, panel_max=vmax, problems=[])
    for b, p in enumerate(R.problems):
        s = p.scale
        entry["problems"].append(dict(
            floor=dict(p.floor, cond=kc.condition(R, b), order_floor=kc.order_floor(R, b)[0], order_panel_max=kc.order_floor(R, b)[1]), scale=s, gate_first=p.gate_first / s,
            first_vs_extended=float(np.abs(dx[b, free] - p.step).max() / s), first_vs_lapack=float(np.abs(dx[b, free] - p.lapack).max() / s),
            first_vs_oracle=float(np.abs(dx[b, free] - p.oracle).max() / s), chord_vs_extended=float(np.abs(dc[b, free] - p.step).max() / s),
            chord_vs_first=float(np.abs(dc[b] - dx[b]).max() / np.abs(dx[b]).max()), refined_vs_extended=float(np.abs(dr[b, free] - p.step).max() / s)))
    kc.record("instantiations", name, entry)
    assert np.isfinite(dx).all() and np.isfinite(dc).all() and np.isfinite(dr).all()
    assert vmax <= kc.GATE_PANEL / cfg.eps_dual, vmax
    for b, p in enumerate(R.problems):
        e, s = entry["problems"][b], p.scale
        assert not dx[b, fixed].any() and not dc[b, fixed].any() and not dr[b, fixed].any(), (name, b)
        assert e["first_vs_extended"] * s <= p.gate_first and e["first_vs_lapack"] * s <= p.gate_first, (name, b, e)
        assert e["first_vs_oracle"] * s <= p.gate_first, (name, b, e)
        assert e["chord_vs_extended"] * s <= p.gate_first, (name, b, e)
        assert e["chord_vs_first"] <= kc.GATE_CHORD, (name, b, e)
        assert e["refined_vs_extended"] <= (kc.GATE_REDUCED if R.reduced else kc.GATE_REFINED), (name, b, e)
    # the three problems have three answers (each was held to a reference of its own above; the references differ by more than
    # a thousand gates: test_kkt_cases_cpu.py)
    for a in range(B):
        for b in range(a + 1, B):
            assert np.abs(dx[a] - dx[b]).max() > 1e2 * max(R.problems[a].gate_first, R.problems[b].gate_first), (name, a, b)
