/* The boolean map of a heightfield made on the device, from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_probe_cpu.py, tests/test_gpu_probe.py): qtos_probe lists the probe patches of one 20 x 20 map with a single raised
 * cell as solver problems -- a first call with capacity 0 reads their number, a second one fills the arrays --, qtos_plan_batch
 * solves them, qtos_probe_stamp writes the boolean map and qtos_path_plan plans one path over it.
 * argv[1]: a QtosParams image written by the Python mirror.  Without a HIP device: the struct size and what the argument checks
 * answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define ROWS 20
#define COLS 20
#define NJ (COLS / 2 - 1)
#define MAX_PROBLEMS 8
#define MAX_PIECES 40
#define MAX_CELLS (2 * MAX_PIECES)

int main(int argc, char **argv) {
  static const double stance[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  static double map[ROWS * COLS], towr[COLS * ROWS], bool_map[ROWS * COLS], knots[MAX_PIECES + 1], coef[8 * MAX_PIECES];
  static int slot[ROWS * NJ], cells[MAX_CELLS * 2];
  QtosParams params;
  QtosDims dims;
  QtosProbe g;
  QtosPathPlan q;
  QtosPlanner *p = NULL;
  double start[MAX_PROBLEMS * QTOS_START_DOUBLES], goal[MAX_PROBLEMS * 3], path_start[QTOS_START_DOUBLES], robot_goal[3], *nodes;
  int offsets[2], patch[MAX_PROBLEMS * 3], map_id[MAX_PROBLEMS], status[MAX_PROBLEMS], n_pieces = -7, n_cells = -7, path_status = -7;
  int rc, rc_dev, rc_stamp, rc_count, n, i, k, e;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  map[10 * COLS + 10] = 0.05;                           /* one raised cell */
  for (i = 1; i < COLS; ++i)                            /* the solver's orientation: [x index][y index], one row on in +x */
    for (k = 0; k < ROWS; ++k) towr[i * ROWS + k] = map[k * COLS + i - 1];
  memset(&g, 0, sizeof(g));
  g.rows = ROWS; g.cols = COLS; g.n_maps = 1; g.cell = 0.1; g.scale = 1; g.multi_map_shift = 1; g.origin_shift = 1.0; g.z_offset = 0.24;
  for (e = 0; e < QTOS_NEE; ++e)
    for (k = 0; k < 3; ++k) g.nominal_stance[e][k] = stance[e][k];
  offsets[0] = offsets[1] = -7;
  for (i = 0; i < MAX_PROBLEMS; ++i) status[i] = map_id[i] = -7;
  rc = qtos_probe(NULL, &g, map, 0, offsets, slot, patch, start, goal, map_id);
  rc_dev = qtos_probe_device(NULL, &g, map, 0, offsets, slot, patch, start, goal, map_id, NULL);
  rc_stamp = qtos_probe_stamp(NULL, &g, offsets, slot, patch, status, bool_map);
  printf("sizeof_probe=%d probe_null=%d probe_device_null=%d probe_stamp_null=%d\n", (int)sizeof(QtosProbe), rc, rc_dev, rc_stamp);
  rc = qtos_planner_create(&params, MAX_PROBLEMS, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0) return 4;
  {  /* the argument checks that need a planner: -2 each, with a reason, and nothing is written */
    QtosProbe w = g;
    int c[6];
    w.cols = 1; c[0] = qtos_probe(p, &w, map, 0, offsets, slot, patch, start, goal, map_id);
    w = g; w.rows = 1025; w.cols = 16; c[1] = qtos_probe(p, &w, map, 0, offsets, slot, patch, start, goal, map_id);
    w = g; w.scale = 5; c[2] = qtos_probe(p, &w, map, 0, offsets, slot, patch, start, goal, map_id);
    w = g; w.cell = 0.0; c[3] = qtos_probe(p, &w, map, 0, offsets, slot, patch, start, goal, map_id);
    c[4] = qtos_probe(p, &g, map, -1, offsets, slot, patch, start, goal, map_id);
    c[5] = qtos_probe_stamp(p, &g, offsets, slot, patch, NULL, bool_map);
    printf("bad_args=%d,%d,%d,%d,%d,%d untouched=%d reason=%d\n", c[0], c[1], c[2], c[3], c[4], c[5], offsets[0] == -7 && offsets[1] == -7,
           strstr(qtos_last_error(p), "qtos_probe") != NULL);
  }
  if (qtos_planner_dims(p, &dims) != 0) return 5;
  nodes = (double *)malloc((size_t)MAX_PROBLEMS * dims.n_vars * sizeof(double));
  if (!nodes) return 5;
  rc = qtos_set_heightfields(p, 1, towr, COLS, ROWS, 0.1, -1.0, -1.0);
  rc_count = rc ? rc : qtos_probe(p, &g, map, 0, offsets, slot, patch, NULL, NULL, NULL);     /* how many problems? */
  n = offsets[1];
  if (rc_count || n < 1 || n > MAX_PROBLEMS) {
    printf("error: count %d n %d %s\n", rc_count, n, qtos_last_error(p));
    return 6;
  }
  rc = qtos_probe(p, &g, map, n, offsets, slot, patch, start, goal, map_id);
  if (!rc) rc = qtos_plan_batch(p, n, start, goal, map_id, NULL, nodes, status, NULL, NULL);
  if (!rc) rc = qtos_probe_stamp(p, &g, offsets, slot, patch, status, bool_map);
  printf("probe=%d n=%d", rc, n);
  for (i = 0; i < n && !rc; ++i)
    printf(" patch%d=%d,%d,%d,%d,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g", i, patch[3 * i], patch[3 * i + 1], patch[3 * i + 2], status[i],
           start[i * QTOS_START_DOUBLES], start[i * QTOS_START_DOUBLES + 1], start[i * QTOS_START_DOUBLES + 2], goal[3 * i], goal[3 * i + 1],
           goal[3 * i + 2]);
  printf("\nbool_map=");
  for (i = 0; i < ROWS * COLS && !rc; ++i) printf("%d", (int)bool_map[i]);
  printf("\n");
  /* one path across the map, over what the stamp left */
  memset(&q, 0, sizeof(q));
  q.rows = ROWS; q.cols = COLS; q.cell = 0.1; q.origin_x = 1.0; q.origin_y = 1.0; q.height_bound = 0.2; q.step_size = 0.25;
  q.max_cells = MAX_CELLS; q.max_open = 1024; q.max_pieces = MAX_PIECES; q.n_maps = 1; q.set_done = 0;
  memset(path_start, 0, sizeof(path_start));
  path_start[0] = -0.85; path_start[1] = 0.05; path_start[2] = 0.24;
  robot_goal[0] = 0.85; robot_goal[1] = 0.05; robot_goal[2] = 0.24;
  if (!rc) rc = qtos_path_plan(p, 1, &q, bool_map, NULL, path_start, robot_goal, knots, coef, &n_pieces, cells, &n_cells, &path_status, NULL);
  printf("path_plan=%d status=%d n_cells=%d n_pieces=%d cells=", rc, path_status, n_cells, n_pieces);
  for (i = 0; i < 2 * MAX_CELLS && !rc; ++i) printf("%s%d", i ? "," : "", cells[i]);
  printf("\n");
  if (rc) printf("error: %d %s\n", rc, qtos_last_error(p));
  free(nodes);
  qtos_planner_destroy(p);
  return rc ? 7 : 0;
}
