/* A randomised terrain made on the device, from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_terrain_env_cpu.py, tests/test_gpu_terrain_env.py): qtos_terrain_env randomises two copies of one 20 x 20 base
 * grid with two raised blocks on two seeds, qtos_set_heightfields installs the solver's orientation of both, qtos_probe lists
 * the probe patches of both maps and qtos_plan_batch solves them, each on its own heightfield.
 * argv[1]: a QtosParams image written by the Python mirror.  Without a HIP device: the struct size and what the argument checks
 * answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define ROWS 20
#define COLS 20
#define NJ (COLS / 2 - 1)
#define N_MAPS 2
#define MAX_PROBLEMS 64

int main(int argc, char **argv) {
  static const double stance[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  static double base[ROWS * COLS], map[N_MAPS * ROWS * COLS], towr[N_MAPS * COLS * ROWS];
  static double start[MAX_PROBLEMS * QTOS_START_DOUBLES], goal[MAX_PROBLEMS * 3];
  static int slot[N_MAPS * ROWS * NJ], patch[MAX_PROBLEMS * 3], map_id[MAX_PROBLEMS], status[MAX_PROBLEMS];
  const unsigned long long seed[N_MAPS] = {7ull, 4294967301ull};
  const int base_id[N_MAPS] = {0, 0};
  QtosParams params;
  QtosDims dims;
  QtosTerrainEnv g;
  QtosProbe q;
  QtosPlanner *p = NULL;
  double *nodes;
  int draws[N_MAPS] = {0, 0}, env_status[N_MAPS] = {-7, -7}, offsets[N_MAPS + 1];
  int rc, rc_dev, rc_set, n, i, k, m, e;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  for (i = 8; i < 11; ++i)
    for (k = 9; k < 12; ++k) base[i * COLS + k] = 0.04;   /* a low block ... */
  base[14 * COLS + 5] = 0.02;                             /* ... and a raised cell: two levels */
  memset(&g, 0, sizeof(g));
  g.n_maps = N_MAPS; g.n_base = 1; g.rows = ROWS; g.cols = COLS; g.n_shift = 3; g.n_height = 10; g.climb = 0; g.delta = 0.005;
  rc = qtos_terrain_env(NULL, &g, base, base_id, seed, draws, map, towr, env_status);
  rc_dev = qtos_terrain_env_device(NULL, &g, base, base_id, seed, draws, map, towr, env_status, NULL);
  rc_set = qtos_set_heightfields_device(NULL, N_MAPS, towr, COLS, ROWS, 0.1, -1.0, -1.0, NULL);
  printf("sizeof_env=%d env_null=%d env_device_null=%d set_device_null=%d\n", (int)sizeof(QtosTerrainEnv), rc, rc_dev, rc_set);
  rc = qtos_planner_create(&params, MAX_PROBLEMS, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0) return 4;
  {  /* the argument checks that need a planner: -2 each, with a reason, and nothing is written */
    QtosTerrainEnv w = g;
    int c[6];
    w.rows = 0; c[0] = qtos_terrain_env(p, &w, base, base_id, seed, draws, map, towr, env_status);
    w = g; w.n_shift = -1; c[1] = qtos_terrain_env(p, &w, base, base_id, seed, draws, map, towr, env_status);
    w = g; w.delta = -0.1; c[2] = qtos_terrain_env(p, &w, base, base_id, seed, draws, map, towr, env_status);
    c[3] = qtos_terrain_env(p, &g, base, base_id, NULL, draws, map, towr, env_status);
    c[4] = qtos_terrain_env(p, &g, base, base_id, seed, draws, base, towr, env_status);
    c[5] = qtos_terrain_env(p, &g, base, NULL, seed, draws, map, towr, env_status);      /* one base, two maps, no base_id */
    printf("bad_args=%d,%d,%d,%d,%d,%d untouched=%d reason=%d\n", c[0], c[1], c[2], c[3], c[4], c[5],
           env_status[0] == -7 && env_status[1] == -7 && draws[0] == 0, strstr(qtos_last_error(p), "qtos_terrain_env") != NULL);
  }
  if (qtos_planner_dims(p, &dims) != 0) return 5;
  nodes = (double *)malloc((size_t)MAX_PROBLEMS * dims.n_vars * sizeof(double));
  if (!nodes) return 5;
  rc = qtos_terrain_env(p, &g, base, base_id, seed, draws, map, towr, env_status);
  printf("terrain_env=%d status=%d,%d draws=%d,%d\n", rc, env_status[0], env_status[1], draws[0], draws[1]);
  for (m = 0; m < N_MAPS && !rc; ++m) {
    printf("map%d=", m);
    for (i = 0; i < ROWS * COLS; ++i)
      if (map[m * ROWS * COLS + i] != 0.0) printf("%d:%.17g,", i, map[m * ROWS * COLS + i]);
    printf(" towr_ok=");
    e = 1;
    for (i = 0; i < COLS; ++i)
      for (k = 0; k < ROWS; ++k) e = e && towr[(m * COLS + i) * ROWS + k] == (i ? map[(m * ROWS + k) * COLS + i - 1] : 0.0);
    printf("%d\n", e);
  }
  if (!rc) rc = qtos_set_heightfields(p, N_MAPS, towr, COLS, ROWS, 0.1, -1.0, -1.0);
  memset(&q, 0, sizeof(q));
  q.rows = ROWS; q.cols = COLS; q.n_maps = N_MAPS; q.cell = 0.1; q.scale = 1; q.multi_map_shift = 1; q.origin_shift = 1.0; q.z_offset = 0.24;
  for (e = 0; e < QTOS_NEE; ++e)
    for (k = 0; k < 3; ++k) q.nominal_stance[e][k] = stance[e][k];
  if (!rc) rc = qtos_probe(p, &q, map, MAX_PROBLEMS, offsets, slot, patch, start, goal, map_id);
  n = rc ? 0 : offsets[N_MAPS];
  if (rc || n < 1 || n > MAX_PROBLEMS) {
    printf("error: probe %d n %d %s\n", rc, n, qtos_last_error(p));
    return 6;
  }
  rc = qtos_plan_batch(p, n, start, goal, map_id, NULL, nodes, status, NULL, NULL);
  printf("plan=%d n=%d offsets=%d,%d,%d status=", rc, n, offsets[0], offsets[1], offsets[2]);
  for (i = 0; i < n && !rc; ++i) printf("%s%d", i ? "," : "", status[i]);
  printf("\n");
  if (rc) printf("error: %d %s\n", rc, qtos_last_error(p));
  free(nodes);
  qtos_planner_destroy(p);
  return rc ? 7 : 0;
}
