/* A receding-horizon loop from plain C99, host pointers only, no HIP and no torch on the caller's side (tests/test_handover_cpu.py,
 * tests/test_gpu_handover.py): one cold qtos_plan_batch of two robots on flat ground, then three times qtos_handover (which row
 * of the plan being executed does the next plan start from, and that row's state: QTOS/combiner.py:245-296) + qtos_plan_batch.
 * argv[1]: a QtosParams image written by the Python mirror.  Without a HIP device: the struct size and what the argument checks
 * answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosHandover h;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], goal_step[NB * 3], offset[NB], viol[NB], *nodes;
  int row[NB], status[NB], iters[NB], rc, rc_dev, b, e, k, r, bad = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  memset(&h, 0, sizeof(h));
  h.advance = 2.5; h.search = 0.4; h.hz = 1000.0;
  h.rule = 1; h.n_heights = 1; h.heights[0] = 0.0;      /* the reference's rule on flat ground */
  h.zero_filter = 1;
  rc = qtos_handover(NULL, NB, &h, start, goal_step, start, goal, offset, row);
  rc_dev = qtos_handover_device(NULL, NB, &h, start, goal_step, start, goal, offset, row, NULL);
  printf("sizeof_handover=%d handover_null=%d handover_device_null=%d\n", (int)sizeof(QtosHandover), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  if (!nodes) return 5;
  {  /* the argument checks that need a planner: -1 each */
    QtosHandover g = h;
    int c[6];
    c[0] = qtos_handover(p, 0, &h, nodes, NULL, start, NULL, offset, row);
    c[1] = qtos_handover(p, NB, &h, nodes, goal_step, start, NULL, offset, row);
    g.n_heights = 9; c[2] = qtos_handover(p, NB, &g, nodes, NULL, start, NULL, offset, row);
    g = h; g.advance = -1.0; c[3] = qtos_handover(p, NB, &g, nodes, NULL, start, NULL, offset, row);
    g = h; g.advance = d.duration + 0.5; c[4] = qtos_handover(p, NB, &g, nodes, NULL, start, NULL, offset, row);
    c[5] = qtos_handover(p, NB + 1, &h, nodes, NULL, start, NULL, offset, row);
    printf("bad_args=%d,%d,%d,%d,%d,%d\n", c[0], c[1], c[2], c[3], c[4], c[5]);
  }
  memset(start, 0, sizeof(start));
  for (b = 0; b < NB; ++b) {      /* at rest in nominal stance, 0.1 m apart; every plan's goal 0.09 m per second of horizon ahead */
    double *s = start + b * QTOS_START_DOUBLES;
    s[0] = 0.1 * b; s[2] = 0.24;
    for (e = 0; e < QTOS_NEE; ++e)
      for (k = 0; k < 3; ++k) s[6 + 3 * e + k] = feet[e][k] + (k == 0 ? s[0] : 0.0);
    goal_step[3 * b] = 0.09 * d.duration; goal_step[3 * b + 1] = goal_step[3 * b + 2] = 0.0;
    goal[3 * b] = s[0] + goal_step[3 * b]; goal[3 * b + 1] = 0.0; goal[3 * b + 2] = 0.24;
  }
  rc = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
  printf("cold rc=%d status=%d,%d iters=%d,%d\n", rc, status[0], status[1], iters[0], iters[1]);
  bad |= rc != 0;
  for (r = 1; r <= 3 && !bad; ++r) {
    rc = qtos_handover(p, NB, &h, nodes, goal_step, start, goal, offset, row);
    if (rc == 0) rc_dev = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
    else rc_dev = rc;
    for (b = 0; b < NB; ++b)
      printf("replan=%d window=%d handover=%d plan=%d row=%d offset=%.3f status=%d iters=%d start=%.17g,%.17g,%.17g goal_x=%.17g\n", r, b, rc,
             rc_dev, row[b], offset[b], status[b], iters[b], start[b * QTOS_START_DOUBLES], start[b * QTOS_START_DOUBLES + 1],
             start[b * QTOS_START_DOUBLES + 2], goal[3 * b]);
    bad |= rc != 0 || rc_dev != 0;
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes);
  qtos_planner_destroy(p);
  return bad ? 6 : 0;
}
