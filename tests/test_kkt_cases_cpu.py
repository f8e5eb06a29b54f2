"""The table of tests/kkt_cases.py against the library's own choice and its source, without a GPU: every case selects the
instantiation it names (capi.analyze_kernel under the case's QTOS_KKT), the table and UNREACHED together are exactly the
instantiations the four selector functions of csrc/qtos_planner.hip compile, and the dense reference of every transcription
stays inside the gates on its own.  A new instantiation without a case, or a case that moved to another kernel behind a change
of the elimination order, fails here."""
import numpy as np
import pytest

import kkt_cases as kc


@pytest.mark.parametrize("name", kc.NAMES)
def test_case_selects_the_instantiation_it_names(name, hip_lib):
    from qtos_amd import capi
    transcription, kkt, kernel, unknowns, stages = kc.CASES[name]
    cfg = kc.config(transcription)
    with kc.kkt_environment(kkt):
        assert capi.analyze_kernel(cfg) == kernel
    with kc.kkt_environment(None):
        d, _ = capi.analyze(cfg)                       # (the default analysis: k_kkt5's pair mode has a front of its own)
    assert (d.n_unknowns, d.n_stages) == (unknowns, stages)
    assert kernel.startswith("k_kkt5") or d.front == kc.kernel_front(kernel)
    assert cfg.reduce_base == cfg.reduce_swing


def test_table_and_unreached_are_the_compiled_set():
    compiled = kc.compiled_instantiations()
    table = kc.table_instantiations()
    assert len(compiled) == 26 + 8 + 4 + 13
    assert not table & set(kc.UNREACHED)
    assert table | set(kc.UNREACHED) == compiled, (sorted(compiled - table - set(kc.UNREACHED)), sorted((table | set(kc.UNREACHED)) - compiled))
    assert len({kc.CASES[n][2] for n in kc.NAMES}) == len(kc.NAMES)          # one case per factor kernel


def test_a_new_instantiation_in_the_source_is_seen():
    """The reader of the selector functions: an instantiation added to the product branch shows up, one added to a development
    branch does not."""
    import os
    text = open(os.path.join(kc.ROOT, "quadruped-trajectory-optimization-stack_amd", "csrc", "qtos_planner.hip")).read()
    product = "switch (F) { QTOS_KKT5(96) QTOS_KKT5(112) QTOS_KKT5(128) QTOS_KKT5(144) }"
    development = "switch (F) { QTOS_KKT5(112) QTOS_KKT5(128) }"
    assert text.count(product) == 1 and text.count(development) == 1
    base = kc.compiled_instantiations(text)
    assert kc.compiled_instantiations(text.replace(product, product.replace("QTOS_KKT5(144)", "QTOS_KKT5(144) QTOS_KKT5(160)"))) == base | {"k_kkt5<160>"}
    assert kc.compiled_instantiations(text.replace(development, development.replace("QTOS_KKT5(128)", "QTOS_KKT5(128) QTOS_KKT5(160)"))) == base


def test_unreached_holds_only_what_no_transcription_selects():
    """At most the small fronts 16, 32 and 64 of k_kkt2 (with and without continuation records) and k_kkt3 with their k_chord, the
    four large k_kkt2 without continuation records, and k_chord<176> / <192> only while their k_kkt2 is unreached."""
    allowed = {k % f for f in (16, 32, 64) for k in ("k_kkt2<%d>", "k_kkt2<%d, true>", "k_kkt3<%d, 1>", "k_chord<%d>")}
    allowed |= {"k_kkt2<%d>" % f for f in (160, 176, 192, 208)}
    for f in (176, 192):
        if "k_kkt2<%d>" % f in kc.UNREACHED and "k_kkt2<%d, true>" % f in kc.UNREACHED:
            allowed.add("k_chord<%d>" % f)
    assert set(kc.UNREACHED) <= allowed, sorted(set(kc.UNREACHED) - allowed)
    for k in kc.UNREACHED:                             # a k_chord is unreached only where every factor kernel of its front is
        if k.startswith("k_chord"):
            f = kc.kernel_front(k)
            assert not any(kc.kernel_front(c) == f for c in kc.table_instantiations() if not c.startswith("k_chord"))


def test_the_table_sits_on_both_sides_of_every_branch():
    """The fronts of the table take both values of every compile-time switch that depends on F, and every MAXT there is."""
    fronts = sorted({kc.kernel_front(kc.CASES[n][2]) for n in kc.NAMES if kc.CASES[n][2].startswith("k_kkt2")})
    assert fronts == list(range(32, 209, 16))
    br = [kc.branches(f) for f in fronts]
    for key in ("VP", "NBUF", "NH"):
        assert len({b[key] for b in br}) == 2, key
    assert {b["NT"] < 12 for b in br} == {True, False} and {b["NU"] >= 12 for b in br} == {True, False}
    assert {b["MAXT"] for b in br} == set(range(1, 8))
    assert kc.branches(96)["NU"] == 12 and kc.branches(128) == dict(NT=8, NTILE=36, NU=12, MAXT=3, NSV=8, VP=True, NBUF=2, NH=2, HN=6, NASM=12)
    for kind, lo, hi in (("k_kkt3", 32, 128), ("k_kkt5", 96, 144)):
        assert sorted(kc.kernel_front(kc.CASES[n][2]) for n in kc.NAMES if kc.CASES[n][2].startswith(kind)) == list(range(lo, hi + 1, 16))
    for cont in (False, True):
        have = {kc.kernel_front(kc.CASES[n][2]) for n in kc.NAMES if kc.CASES[n][2].startswith("k_kkt2") and kc.CASES[n][2].endswith("true>") == cont}
        assert have == set(range(48 if cont else 32, 209, 16))


@pytest.mark.parametrize("transcription", list(kc.TRANSCRIPTIONS))
def test_the_reference_alone_is_inside_the_gates(transcription):
    """The floor of the reference: the extended-precision refinement has converged a thousand times below the tightest gate,
    LAPACK in float64 is within a tenth of the first-solve gate of it, at a reduced system's point the full system's eps_dual on
    the eliminated rows moves the step by no more than half the gate of a reduced step, on a full system a float64 block
    elimination in the planner's order loses no more than a fifth of the first-solve gate and keeps its panels within the
    panel gate, and the three problems' steps differ from each other by
    more than a thousand first-solve gates -- a kernel that solved problem 0 for all three fails every gate."""
    assert any(kc.CASES[n][0] == transcription for n in kc.NAMES)
    R = kc.reference(transcription)
    for b, p in enumerate(R.problems):
        assert p.floor["last_correction"] <= 1e-3 * kc.GATE_REFINED, (b, p.floor)
        assert p.floor["lapack_vs_extended"] <= 0.1 * kc.GATE_FIRST, (b, p.floor)
        assert kc.GATE_FIRST * p.scale <= p.gate_first <= kc.GATE_SPREAD_FACTOR * 1.5e-6 * p.scale, (b, p.floor)
        assert np.isfinite(p.step).all() and p.scale > 0
        assert ("reduced_vs_full" in p.floor) == R.reduced
        if R.reduced:                                  # (half the gate is the reference's, half the kernel's)
            assert p.floor["reduced_vs_full"] <= 0.5 * kc.GATE_REDUCED, (b, p.floor)
        else:                                          # (a fifth of the gate is the method's, the rest the kernel's)
            err, vmax = kc.order_floor(R, b)
            assert err * p.scale <= 0.2 * p.gate_first and vmax <= kc.GATE_PANEL / R.cfg.eps_dual, (b, err, vmax)
    for a in range(kc.B):
        for b in range(a + 1, kc.B):
            gap = np.abs(R.problems[a].step - R.problems[b].step).max()
            assert gap > 1e3 * max(R.problems[a].gate_first, R.problems[b].gate_first), (a, b, gap)
