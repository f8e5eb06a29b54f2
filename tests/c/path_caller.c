/* Receding windows that follow a global path, from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_path_goal_cpu.py, tests/test_gpu_path_goal.py): the first goal is qtos_path_goal's step from the start state
 * (Combiner.plan_init), then three times qtos_handover (where the next plan starts) + qtos_path_goal (where it goes: the path one
 * horizon ahead of the hand-over, Global_Planner.update) + qtos_plan_batch.  Two windows on one two-piece path over flat ground;
 * window 1 is so far along it that the path's end falls behind it in the third replan: its done bit 0 is set and it is held.
 * argv[1]: a QtosParams image written by the Python mirror.  Without a HIP device: the struct size and what the argument checks
 * answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define NPIECES 2

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  /* x(t) = 0.08 t; y a C2 cubic: 2e-5 t^3 up to t = 10, then 0.02 + 0.006 s + 0.0006 s^2 - 2e-5 s^3, s = t - 10 */
  static const double knots[NPIECES + 1] = {0.0, 10.0, 20.0};
  static const double coef[2 * 4 * NPIECES] = {0.0,  0.0,   0.0, 0.0,    0.08, 0.08,  0.0, 0.8,       /* X: c[k][i], k = 0 .. 3 */
                                               2e-5, -2e-5, 0.0, 0.0006, 0.0,  0.006, 0.0, 0.02};     /* Y */
  static const int n_pieces[1] = {NPIECES};
  static const int path_id[NB] = {0, 0};
  static const double first_clock[NB] = {0.0, 21.0};
  static const double first_xy[NB][2] = {{0.0, 0.0}, {1.68, 0.13}};
  QtosParams params;
  QtosDims d;
  QtosHandover h;
  QtosPathGoal g;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], offset[NB], clock[NB], viol[NB], *nodes;
  int row[NB], status[NB], iters[NB], done[NB], rc, rc_dev, rc_goal, b, e, k, r, bad = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  memset(&h, 0, sizeof(h));
  h.advance = 2.5; h.search = 0.4; h.hz = 1000.0;
  h.rule = 1; h.n_heights = 1; h.heights[0] = 0.0;      /* the reference's rule on flat ground */
  h.zero_filter = 1;
  memset(&g, 0, sizeof(g));
  g.horizon = 5.0; g.step_size = 0.45; g.tol = 1e-5; g.z_offset = 0.24;
  g.cell = 0.1; g.origin_x = 1.0; g.origin_y = 1.0;
  g.t_stop = 5.0 + h.advance; g.stop_dist = 0.0;
  g.base = 1; g.clamp_x = 0; g.advance_clock = 1; g.hold_done = 1;
  g.n_paths = 1; g.max_pieces = NPIECES;
  memset(start, 0, sizeof(start));
  rc = qtos_path_goal(NULL, NB, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
  rc_dev = qtos_path_goal_device(NULL, NB, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done, NULL);
  printf("sizeof_path_goal=%d path_goal_null=%d path_goal_device_null=%d\n", (int)sizeof(QtosPathGoal), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  if (!nodes) return 5;
  for (b = 0; b < NB; ++b) {      /* at rest in nominal stance on the path */
    double *s = start + b * QTOS_START_DOUBLES;
    s[0] = first_xy[b][0]; s[1] = first_xy[b][1]; s[2] = 0.24;
    for (e = 0; e < QTOS_NEE; ++e)
      for (k = 0; k < 3; ++k) s[6 + 3 * e + k] = feet[e][k] + (k < 2 ? s[k] : 0.0);
    clock[b] = first_clock[b];
    done[b] = 0;
    goal[3 * b] = goal[3 * b + 1] = goal[3 * b + 2] = -1.0;
  }
  {  /* the argument checks that need a planner: -1 each, and nothing is written */
    QtosPathGoal q = g;
    int c[8];
    c[0] = qtos_path_goal(p, 0, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    c[1] = qtos_path_goal(p, NB, &g, knots, coef, n_pieces, NULL, NULL, NULL, NULL, clock, NULL, start, goal, done);   /* n_paths < B */
    q.max_pieces = 0; c[2] = qtos_path_goal(p, NB, &q, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    q = g; q.cell = 0.0; c[3] = qtos_path_goal(p, NB, &q, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    q = g; q.step_size = -0.1; c[4] = qtos_path_goal(p, NB, &q, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    q = g; q.base = 2; c[5] = qtos_path_goal(p, NB, &q, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    q = g; q.clamp_x = 1; c[6] = qtos_path_goal(p, NB, &q, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
    c[7] = qtos_path_goal(p, NB, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, NULL);  /* hold_done without done */
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d untouched=%d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7],
           goal[0] == -1.0 && goal[5] == -1.0 && clock[1] == first_clock[1] && done[0] == 0);
  }
  /* plan_init: the first goal is the clipped step from the start state towards the path one horizon ahead */
  rc_goal = qtos_path_goal(p, NB, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, NULL, start, goal, done);
  rc = rc_goal ? rc_goal : qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
  for (b = 0; b < NB; ++b)
    printf("replan=0 window=%d handover=0 path_goal=%d plan=%d row=0 offset=%.17g clock=%.17g done=%d status=%d iters=%d start=%.17g,%.17g,%.17g "
           "goal=%.17g,%.17g,%.17g\n", b, rc_goal, rc, 0.0, clock[b], done[b], status[b], iters[b], start[b * QTOS_START_DOUBLES],
           start[b * QTOS_START_DOUBLES + 1], start[b * QTOS_START_DOUBLES + 2], goal[3 * b], goal[3 * b + 1], goal[3 * b + 2]);
  bad |= rc != 0;
  g.base = 0;                     /* from here on Global_Planner.update: the step is taken from the spine at the plan's start */
  for (r = 1; r <= 3 && !bad; ++r) {
    rc = qtos_handover(p, NB, &h, nodes, NULL, start, NULL, offset, row);
    rc_goal = rc ? rc : qtos_path_goal(p, NB, &g, knots, coef, n_pieces, NULL, path_id, NULL, NULL, clock, offset, start, goal, done);
    rc_dev = rc_goal ? rc_goal : qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
    for (b = 0; b < NB; ++b)
      printf("replan=%d window=%d handover=%d path_goal=%d plan=%d row=%d offset=%.17g clock=%.17g done=%d status=%d iters=%d "
             "start=%.17g,%.17g,%.17g goal=%.17g,%.17g,%.17g\n", r, b, rc, rc_goal, rc_dev, row[b], offset[b], clock[b], done[b], status[b],
             iters[b], start[b * QTOS_START_DOUBLES], start[b * QTOS_START_DOUBLES + 1], start[b * QTOS_START_DOUBLES + 2], goal[3 * b],
             goal[3 * b + 1], goal[3 * b + 2]);
    bad |= rc != 0 || rc_goal != 0 || rc_dev != 0;
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes);
  qtos_planner_destroy(p);
  return bad ? 6 : 0;
}
