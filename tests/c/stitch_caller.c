/* The executed trajectory of a receding-horizon loop from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_stitch_cpu.py, tests/test_gpu_stitch.py): one cold qtos_plan_batch of two robots on flat ground, then three times
 * qtos_handover (the row the next plan starts from) + qtos_stitch (the rows executed up to it go to the window's ring, its clock
 * moves on: Combiner.combine, QTOS/combiner.py:125-135) + qtos_plan_batch, and at the end the rest of the newest plan.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints every window's cursor and the time stamps of its first and
 * last ring row; exit status 7 if a window's time stamps do not increase.  Without a HIP device: the struct size and what the
 * argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define CAPACITY 16000   /* 3 x at most 2901 rows + the 5001 rows of the last plan */

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosHandover h;
  QtosStitch s;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], goal_step[NB * 3], offset[NB], viol[NB], t0[NB], *nodes, *traj;
  long long cursor[NB], j;
  int row[NB], status[NB], iters[NB], rc, rc_dev, b, e, k, r, bad = 0, order = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  memset(&h, 0, sizeof(h));
  h.advance = 2.5; h.search = 0.4; h.hz = 1000.0;
  h.rule = 1; h.n_heights = 1; h.heights[0] = 0.0;      /* the reference's rule on flat ground */
  h.zero_filter = 1;
  memset(&s, 0, sizeof(s));
  s.hz = 1000.0; s.first_row = 0; s.advance_clock = 1; s.capacity = CAPACITY;
  rc = qtos_stitch(NULL, NB, &s, start, row, t0, start, cursor);
  rc_dev = qtos_stitch_device(NULL, NB, &s, start, row, t0, start, cursor, NULL);
  printf("sizeof_stitch=%d stitch_null=%d stitch_device_null=%d\n", (int)sizeof(QtosStitch), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  traj = (double *)calloc((size_t)NB * CAPACITY * QTOS_CSV_COLS, sizeof(double));
  if (!nodes || !traj) return 5;
  {  /* the argument checks that need a planner: -1 each */
    QtosStitch g = s;
    int c[6];
    c[0] = qtos_stitch(p, 0, &s, nodes, row, t0, traj, cursor);
    c[1] = qtos_stitch(p, NB, &s, nodes, row, NULL, traj, cursor);
    g.capacity = 0; c[2] = qtos_stitch(p, NB, &g, nodes, row, t0, traj, cursor);
    g = s; g.first_row = -1; c[3] = qtos_stitch(p, NB, &g, nodes, row, t0, traj, cursor);
    g = s; g.first_row = 1000001; c[4] = qtos_stitch(p, NB, &g, nodes, row, t0, traj, cursor);
    g = s; g.n_rows = -1; c[5] = qtos_stitch(p, NB, &g, nodes, NULL, t0, traj, cursor);
    printf("bad_args=%d,%d,%d,%d,%d,%d\n", c[0], c[1], c[2], c[3], c[4], c[5]);
  }
  memset(start, 0, sizeof(start));
  for (b = 0; b < NB; ++b) {      /* at rest in nominal stance, 0.1 m apart; every plan's goal 0.09 m per second of horizon ahead */
    double *st = start + b * QTOS_START_DOUBLES;
    st[0] = 0.1 * b; st[2] = 0.24;
    for (e = 0; e < QTOS_NEE; ++e)
      for (k = 0; k < 3; ++k) st[6 + 3 * e + k] = feet[e][k] + (k == 0 ? st[0] : 0.0);
    goal_step[3 * b] = 0.09 * d.duration; goal_step[3 * b + 1] = goal_step[3 * b + 2] = 0.0;
    goal[3 * b] = st[0] + goal_step[3 * b]; goal[3 * b + 1] = 0.0; goal[3 * b + 2] = 0.24;
    t0[b] = 10.0 * b;             /* the windows' clocks start apart */
    cursor[b] = 0;
  }
  rc = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
  printf("cold rc=%d status=%d,%d iters=%d,%d\n", rc, status[0], status[1], iters[0], iters[1]);
  bad |= rc != 0;
  for (r = 1; r <= 3 && !bad; ++r) {
    int rc_st = -9, rc_plan = -9;
    rc = qtos_handover(p, NB, &h, nodes, goal_step, start, goal, offset, row);
    if (rc == 0) rc_st = qtos_stitch(p, NB, &s, nodes, row, t0, traj, cursor);      /* the plan handed over from, up to its row[b] */
    if (rc_st == 0) rc_plan = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
    for (b = 0; b < NB; ++b)
      printf("replan=%d window=%d handover=%d stitch=%d plan=%d row=%d cursor=%lld t0=%.17g status=%d\n", r, b, rc, rc_st, rc_plan, row[b],
             cursor[b], t0[b], status[b]);
    bad |= rc != 0 || rc_st != 0 || rc_plan != 0;
  }
  if (!bad) {                     /* the rest of the newest plan: every row, the same count for both windows */
    QtosStitch g = s;
    g.n_rows = (int)(d.duration * s.hz + 0.5) + 1;
    g.advance_clock = 0;
    rc = qtos_stitch(p, NB, &g, nodes, NULL, t0, traj, cursor);
    bad |= rc != 0;
    printf("finish rc=%d rows=%d\n", rc, g.n_rows);
  }
  for (b = 0; b < NB && !bad; ++b) {
    const double *ring = traj + (size_t)b * CAPACITY * QTOS_CSV_COLS;
    int inc = cursor[b] >= 1 && cursor[b] <= CAPACITY;
    for (j = 1; inc && j < cursor[b]; ++j) inc = ring[j * QTOS_CSV_COLS] > ring[(j - 1) * QTOS_CSV_COLS];
    printf("window=%d cursor=%lld first_t=%.17g last_t=%.17g increasing=%d\n", b, cursor[b], ring[0],
           inc ? ring[(cursor[b] - 1) * QTOS_CSV_COLS] : 0.0, inc);
    order |= !inc;
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes);
  free(traj);
  qtos_planner_destroy(p);
  return bad ? 6 : (order ? 7 : 0);
}
