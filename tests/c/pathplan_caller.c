/* Global paths planned on the device, from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_path_plan_cpu.py, tests/test_gpu_path_plan.py): qtos_path_plan plans the paths of three windows over one 10 x 16
 * boolean map with a wall across it -- a detour round the wall, a straight row, and a goal outside the grid, which has no path --
 * and qtos_path_goal then takes one step from the table it wrote (Combiner.plan_init: from the start state, at clock 0).
 * argv[1]: a QtosParams image written by the Python mirror.  Without a HIP device: the struct size and what the argument checks
 * answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 3
#define ROWS 10
#define COLS 16
#define MAX_PIECES 20
#define MAX_CELLS (2 * MAX_PIECES)

int main(int argc, char **argv) {
  static const double first_xy[NB][2] = {{-0.85, -0.55}, {-0.85, -0.95}, {-0.85, -0.55}};
  static const double goals[NB][3] = {{0.45, -0.45, 0.24}, {0.45, -0.95, 0.24}, {1.45, -0.45, 0.24}};
  static double map[ROWS * COLS], knots[NB * (MAX_PIECES + 1)], coef[NB * 8 * MAX_PIECES];
  static int cells[NB * MAX_CELLS * 2];
  QtosParams params;
  QtosPathPlan g;
  QtosPathGoal q;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], robot_goal[NB * 3], clock[NB], goal[NB * 3];
  int n_pieces[NB], n_cells[NB], status[NB], done[NB], rc, rc_dev, rc_goal, b, i, k;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  for (i = 1; i < 8; ++i) map[i * COLS + 7] = 1.0;      /* the wall: column 7, rows 1 .. 7 */
  memset(&g, 0, sizeof(g));
  g.rows = ROWS; g.cols = COLS; g.cell = 0.1; g.origin_x = 1.0; g.origin_y = 1.0;
  g.height_bound = 0.2; g.step_size = 0.25;
  g.max_cells = MAX_CELLS; g.max_open = 256; g.max_pieces = MAX_PIECES; g.n_maps = 1; g.set_done = 1;
  memset(start, 0, sizeof(start));
  for (b = 0; b < NB; ++b) {
    start[b * QTOS_START_DOUBLES] = first_xy[b][0];
    start[b * QTOS_START_DOUBLES + 1] = first_xy[b][1];
    start[b * QTOS_START_DOUBLES + 2] = 0.24;
    for (k = 0; k < 3; ++k) robot_goal[3 * b + k] = goals[b][k];
    clock[b] = 0.0;
    done[b] = 0;
    n_cells[b] = status[b] = -7;
  }
  rc = qtos_path_plan(NULL, NB, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
  rc_dev = qtos_path_plan_device(NULL, NB, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done, NULL);
  printf("sizeof_path_plan=%d path_plan_null=%d path_plan_device_null=%d\n", (int)sizeof(QtosPathPlan), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0) return 4;
  {  /* the argument checks that need a planner: -2 each, with a reason, and nothing is written */
    QtosPathPlan w = g;
    int c[9];
    c[0] = qtos_path_plan(p, 0, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w.rows = 1025; w.cols = 16; c[1] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w = g; w.max_open = 4097; c[2] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w = g; w.max_cells = 2 * MAX_PIECES + 1; c[3] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w = g; w.cell = 0.0; c[4] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w = g; w.step_size = 0.0; c[5] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    w = g; w.n_maps = 0; c[6] = qtos_path_plan(p, NB, &w, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
    c[7] = qtos_path_plan(p, NB, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, NULL);   /* set_done without done */
    c[8] = qtos_path_plan(p, NB, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, NULL, status, done);
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d,%d untouched=%d reason=%d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8],
           status[0] == -7 && n_cells[NB - 1] == -7 && done[0] == 0, strstr(qtos_last_error(p), "qtos_path_plan") != NULL);
  }
  rc = qtos_path_plan(p, NB, &g, map, NULL, start, robot_goal, knots, coef, n_pieces, cells, n_cells, status, done);
  /* one step from the table: window b follows path b */
  memset(&q, 0, sizeof(q));
  q.horizon = 5.0; q.step_size = g.step_size; q.tol = 1e-5; q.z_offset = 0.24;
  q.cell = g.cell; q.origin_x = g.origin_x; q.origin_y = g.origin_y;
  q.t_stop = 7.5; q.stop_dist = 0.0;
  q.base = 1; q.clamp_x = 1; q.advance_clock = 1; q.hold_done = 1;
  q.n_paths = NB; q.max_pieces = MAX_PIECES;
  rc_goal = rc ? rc : qtos_path_goal(p, NB, &q, knots, coef, n_pieces, robot_goal, NULL, NULL, NULL, clock, NULL, start, goal, done);
  for (b = 0; b < NB && !rc && !rc_goal; ++b) {
    printf("window=%d path_plan=%d path_goal=%d status=%d n_cells=%d n_pieces=%d done=%d goal=%.17g,%.17g,%.17g knots=", b, rc, rc_goal,
           status[b], n_cells[b], n_pieces[b], done[b], goal[3 * b], goal[3 * b + 1], goal[3 * b + 2]);
    for (i = 0; i <= MAX_PIECES; ++i) printf("%s%.17g", i ? "," : "", knots[b * (MAX_PIECES + 1) + i]);
    printf(" coef=");
    for (i = 0; i < 8 * MAX_PIECES; ++i) printf("%s%.17g", i ? "," : "", coef[b * 8 * MAX_PIECES + i]);
    printf(" cells=");
    for (i = 0; i < 2 * MAX_CELLS; ++i) printf("%s%d", i ? "," : "", cells[b * 2 * MAX_CELLS + i]);
    printf("\n");
  }
  if (rc || rc_goal) printf("error: %d %d %s\n", rc, rc_goal, qtos_last_error(p));
  qtos_planner_destroy(p);
  return rc || rc_goal ? 6 : 0;
}
