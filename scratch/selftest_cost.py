"""Cost of the create-time KKT self-test (profiles/selftest_cost.json): wall time of a plain create, of a
checked create whose first candidate passes, and QtosSelftest.seconds, for four transcriptions -- N creates each in one process,
plain and checked alternating, medians.  Usage: python scratch/selftest_cost.py [out.json] [N]"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qtos_amd import capi                      # noqa: E402
from qtos_amd.config import PlannerConfig      # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "selftest_cost.json"
N = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cases = {"knots100_trot": PlannerConfig.knots100(gait="trot"), "knots100_walk": PlannerConfig.knots100(),
         "knots200": PlannerConfig.knots200(), "walk_28s": PlannerConfig(gait="walk", duration=28.0)}
capi.Planner(cases["knots100_trot"], max_batch=2).close()      # (the process's first create loads the code object)
res = {}
for name, cfg in cases.items():
    plain, checked, test = [], [], []
    for _ in range(N):
        t0 = time.perf_counter()
        P = capi.Planner(cfg, max_batch=2)
        t1 = time.perf_counter()
        P.close()
        t2 = time.perf_counter()
        Q = capi.Planner(cfg, max_batch=2, checked=True)
        t3 = time.perf_counter()
        assert len(Q.selftests) == 1 and Q.selftests[0].passed
        test.append(Q.selftests[0].seconds)
        dims = Q.dims
        Q.close()
        plain.append(t1 - t0)
        checked.append(t3 - t2)
    med = statistics.median
    res[name] = dict(order_rule=dims.order_rule, front=dims.front, n_stages=dims.n_stages, creates=N,
                     plain_create_ms=round(1e3 * med(plain), 2), checked_create_ms=round(1e3 * med(checked), 2),
                     selftest_ms=round(1e3 * med(test), 3), ratio=round(med(checked) / med(plain), 4),
                     plain_create_ms_all=[round(1e3 * v, 2) for v in plain], checked_create_ms_all=[round(1e3 * v, 2) for v in checked],
                     selftest_ms_all=[round(1e3 * v, 3) for v in test])
    print(name, res[name])
with open(out, "w") as fh:
    json.dump(dict(what="medians of %d creates each, one process, max_batch 2, plain and checked alternating; MI355X" % N, cases=res), fh, indent=1)
    fh.write("\n")
