"""bench.py's command line on the CPU: the defaults the driver relies on, and every bench command README.md prints parses
(the eight-GPU commands of BASELINE configs[3] / configs[4] are the driver's to run; here they must at least be commands),
--dump-outputs, and on the GPU the number of timed steps and the dumped plans."""
import os
import re
import shlex
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_defaults_are_the_headline_run():
    import bench
    a = bench.parse_args([])
    assert (a.gpus, a.steps, a.warmup, a.batch) == (1, 100, 5, 256)
    # the line's metric / value / roofline are the TROT's (the gait BASELINE.json's metric names); the walk of the reference's golden
    # plans is the second leg of the same command, timed with the same --steps
    assert (a.transcription, a.gait, a.workload) == ("knots100", "trot", "exp1_flat")
    assert not a.no_second_gait and not hasattr(a, "trot_steps")
    assert a.settle == 50 and a.settle_tol == 0.02 and not a.no_pattern     # adaptive warm-up on, launch pattern on
    assert a.events_every == 4     # per-kernel HIP events on every fourth timed step (they cost a batch 1.9 %)
    # the terrain workloads and the receding windows keep the walk (their goals, schedules and parity tests are the walk's)
    assert bench.parse_args(["--workload", "exp5_step"]).gait == "walk"
    assert bench.parse_args(["--workload", "mixed"]).gait == "walk"
    assert bench.parse_args(["--transcription", "knots200", "--workload", "mpc_random"]).gait == "walk"
    assert bench.parse_args(["--gait", "walk"]).gait == "walk" and bench.parse_args(["--no-trot"]).no_second_gait
    assert not a.full_system and not a.full_swings and not a.plain_mu and not a.force_torchrun
    assert a.cpu_sample > 0 and not a.no_parity


def test_readme_bench_commands_parse():
    import bench
    text = open(os.path.join(ROOT, "README.md")).read()
    cmds = [l.strip() for l in text.splitlines() if l.startswith("    python ") and "bench.py" in l]
    assert len(cmds) >= 3
    seen = set()
    for c in cmds:
        argv = shlex.split(c.split("#")[0])
        argv = argv[argv.index("bench.py") + 1:]
        a = bench.parse_args(argv)
        seen.add((a.gpus, a.workload, a.transcription))
        if "torch.distributed.run" in c:   # the launcher's process count is the --gpus the ranks are told
            assert re.search(r"--nproc-per-node (\d+)", c).group(1) == str(a.gpus) and "--master-addr 127.0.0.1" in c
    # BASELINE configs[3]: batch 2048 mixed terrains over 8 GPUs; configs[4]: 200-knot receding windows over 8 GPUs
    assert (8, "mixed", "knots100") in seen and (8, "mpc_random", "knots200") in seen


def test_steps_must_be_positive_and_dump_outputs_parses():
    import bench
    assert bench.parse_args([]).dump_outputs is None
    assert bench.parse_args(["--steps", "7", "--dump-outputs", "out"]).dump_outputs == "out"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


def test_dump_outputs_writes_float64_and_samples_above_the_limit(tmp_path):
    """--dump-outputs: whole arrays in float64 below the limit; above it the same seeded rows of every array (their indices in
    sample_rows.npy), the files together within the limit, and the same rows on every call."""
    import numpy as np
    import bench
    rng = np.random.default_rng(5)
    arrays = {"nodes": rng.random((300, 500)), "status": np.zeros(300, np.int32), "iterations": np.full(300, 4, np.int32),
              "violation": rng.random(300) * 1e-5}
    small = tmp_path / "small"
    bench.dump_outputs(str(small), arrays)
    assert sorted(p.name for p in small.iterdir()) == ["iterations.npy", "nodes.npy", "status.npy", "violation.npy"]
    for name, a in arrays.items():
        got = np.load(small / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, a)
    limit = 400_000
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
        assert sum(p.stat().st_size for p in (tmp_path / d).iterdir()) <= limit
    rows = np.load(tmp_path / "big1" / "sample_rows.npy").astype(int)
    assert 0 < len(rows) < 300 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "big1" / "nodes.npy"), arrays["nodes"][rows])
    assert np.array_equal(np.load(tmp_path / "big1" / "violation.npy"), arrays["violation"][rows])
    for p in (tmp_path / "big1").iterdir():
        assert np.array_equal(np.load(p), np.load(tmp_path / "big2" / p.name))
    # a later whole dump into the same directory drops the stale row indices
    bench.dump_outputs(str(tmp_path / "big1"), arrays)
    assert not (tmp_path / "big1" / "sample_rows.npy").exists()


@pytest.mark.gpu
def test_bench_times_exactly_steps_and_dumps_the_same_outputs_every_run(tmp_path):
    """`--steps K` times K steps (`steps`, `plans_timed`, `ms_per_step` on the line) and --dump-outputs writes the plans of the
    last timed step: the ones the planner returns for that step's seeded batch, identical from run to run."""
    import json
    import subprocess
    import numpy as np
    from qtos_amd import workloads
    from qtos_amd.capi import Planner
    from qtos_amd.config import PlannerConfig
    steps, warmup = 3, 2
    outs = []
    for k in range(2):
        d = tmp_path / ("dump%d" % k)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", str(warmup),
                            "--cpu-sample", "0", "--no-parity", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
        assert line["steps"] == steps and line["config"]["plans_timed"] == steps * 256 and len(line["step_ms_series"]) == steps
        # (both figures are rounded to 1e-4 on the line: of ms and of s)
        assert abs(line["ms_per_step"] - 1e3 * line["timed_region_s"] / steps) <= 1e-4 + 1e3 * 5e-5 / steps
        assert line["walk"]["steps"] == steps and len(line["walk"]["step_ms_series"]) == steps
        outs.append({p.name: np.load(p) for p in d.iterdir()})
    assert sorted(outs[0]) == sorted(n + ".npy" for g in ("", "walk_") for n in (g + "nodes", g + "status", g + "iterations", g + "violation"))
    for name, a in outs[0].items():
        assert a.dtype == np.float64 and np.array_equal(a, outs[1][name]), name
    # the last timed step's batch is seeded batch warmup + steps - 1 (bench.py `seeded`): re-solved here, the same plans
    P = Planner(PlannerConfig.knots100(gait="trot"), max_batch=256)
    P.set_heightfields(*workloads.exp1_terrain())
    start, goal = workloads.flat_goals(256, seed=1000 * (warmup + steps - 1))
    nodes, status, iters, viol = P.plan(start, goal)
    P.close()
    assert (status == 0).all()
    assert np.array_equal(outs[0]["nodes.npy"], nodes) and np.array_equal(outs[0]["status.npy"], status)
    assert np.array_equal(outs[0]["iterations.npy"], iters) and np.array_equal(outs[0]["violation.npy"], viol)
