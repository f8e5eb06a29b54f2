/* Joint commands of a plan from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_joint_caller.py, tests/test_gpu_joints.py): one cold qtos_plan_batch of two robots on flat ground, qtos_sample_csv of
 * its rows, qtos_joint_rows of the same rows (table mode), and one 1 kHz tick: a row of its own per robot, with a measured state.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints what the test compares; exit status 7 if a time stamp of
 * the joint table differs from the CSV table's, 8 if the tick is not the table's row where it must be.  Without a HIP device:
 * the struct size and what the argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 200.0
#define NROWS 1001

static void solo12(QtosJointRows *g) {
  static const double hip[QTOS_NEE][3] = {{0.1946, 0.08750000000000001, 0.0}, {0.1946, -0.08750000000000001, 0.0}, {-0.1946, 0.08750000000000001, 0.0}, {-0.1946, -0.08750000000000001, 0.0}};
  int e, k;      /* (the URDF's own digits: joints.SOLO12) */
  memset(g, 0, sizeof(*g));
  g->hz = HZ; g->ee_shift = 0.015; g->l_upper = g->l_lower = 0.16; g->tau_max = 8.0;
  for (e = 0; e < QTOS_NEE; ++e) {
    for (k = 0; k < 3; ++k) g->hip[e][k] = hip[e][k];
    g->lateral[e] = (e % 2 ? -1.0 : 1.0) * (0.014 + 0.037450000000000004 + 0.008);
    g->knee_sign[e] = e < 2 ? -1.0 : 1.0;
  }
  for (k = 0; k < 12; ++k) { g->kp[k] = 20.0; g->kd[k] = 0.08; }
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosJointRows g, t;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB], q_mes[NB * 12], qd_mes[NB * 12], tick[NB * QTOS_CSV_COLS];
  double *nodes, *rows, *joint;
  int status[NB], iters[NB], first[NB], tick_status[NB], *jstatus, rc, rc_dev, b, e, k, bad = 0, stamps = 0, ticks = 0, flagged = 0, clipped = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  solo12(&g);
  g.n_rows = NROWS;
  rc = qtos_joint_rows(NULL, NB, &g, start, t0, NULL, NULL, NULL, NULL, NULL, start, status);
  rc_dev = qtos_joint_rows_device(NULL, NB, &g, start, t0, NULL, NULL, NULL, NULL, NULL, start, status, NULL);
  printf("sizeof_joint_rows=%d joint_null=%d joint_device_null=%d\n", (int)sizeof(QtosJointRows), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  rows = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  joint = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  jstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !rows || !joint || !jstatus) return 5;
  {  /* the argument checks that need a planner: -1 each */
    long long cur[NB] = {0, 0};
    int c[8];
    c[0] = qtos_joint_rows(p, 0, &g, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    c[1] = qtos_joint_rows(p, NB, &g, nodes, NULL, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    t = g; t.capacity = 8; c[2] = qtos_joint_rows(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);   /* a ring without cursor */
    t = g; t.capacity = -1; c[3] = qtos_joint_rows(p, NB, &t, nodes, t0, NULL, NULL, cur, NULL, NULL, joint, jstatus);
    t = g; t.n_rows = 0; c[4] = qtos_joint_rows(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    t = g; t.first_row = 1000001; c[5] = qtos_joint_rows(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    c[6] = qtos_joint_rows(p, NB, &g, nodes, t0, NULL, NULL, NULL, q_mes, NULL, joint, jstatus);
    t = g; t.l_lower = 0.0; c[7] = qtos_joint_rows(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
  }
  memset(start, 0, sizeof(start));
  for (b = 0; b < NB; ++b) {      /* at rest in nominal stance, 0.1 m apart; the goal 0.09 m per second of horizon ahead */
    double *st = start + b * QTOS_START_DOUBLES;
    st[0] = 0.1 * b; st[2] = 0.24;
    for (e = 0; e < QTOS_NEE; ++e)
      for (k = 0; k < 3; ++k) st[6 + 3 * e + k] = feet[e][k] + (k == 0 ? st[0] : 0.0);
    goal[3 * b] = st[0] + 0.09 * d.duration; goal[3 * b + 1] = 0.0; goal[3 * b + 2] = 0.24;
    t0[b] = 10.0 * b;
  }
  rc = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
  printf("plan rc=%d status=%d,%d\n", rc, status[0], status[1]);
  bad |= rc != 0;
  if (!bad) {
    rc = qtos_sample_csv(p, NB, nodes, t0, HZ, NROWS, rows);
    rc_dev = qtos_joint_rows(p, NB, &g, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    bad |= rc != 0 || rc_dev != 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        stamps += joint[((size_t)b * NROWS + k) * QTOS_CSV_COLS] != rows[((size_t)b * NROWS + k) * QTOS_CSV_COLS];
        flagged += jstatus[(size_t)b * NROWS + k] != 0;
      }
    printf("sample rc=%d joint rc=%d stamp_mismatches=%d flagged_rows=%d\n", rc, rc_dev, stamps, flagged);
  }
  if (!bad) {                     /* one tick: robot b at its row 100 + 150 b; robot 0 measures the command itself, robot 1 is far off */
    t = g; t.n_rows = 1;
    for (b = 0; b < NB; ++b) {
      const double *jr;
      first[b] = 100 + 150 * b;
      jr = joint + ((size_t)b * NROWS + first[b]) * QTOS_CSV_COLS;
      for (k = 0; k < 12; ++k) {
        q_mes[12 * b + k] = jr[1 + k] + (b ? 1.0 : 0.0);
        qd_mes[12 * b + k] = jr[13 + k];
      }
    }
    rc = qtos_joint_rows(p, NB, &t, nodes, t0, first, NULL, NULL, q_mes, qd_mes, tick, tick_status);
    bad |= rc != 0;
    for (b = 0; b < NB && !bad; ++b) {
      const double *jr = joint + ((size_t)b * NROWS + first[b]) * QTOS_CSV_COLS, *tk = tick + b * QTOS_CSV_COLS;
      for (k = 0; k < 25; ++k) ticks += tk[k] != jr[k];                              /* stamp, q, qdot: the table's */
      for (k = 25; k < 37; ++k) {
        if (b == 0) ticks += tk[k] != jr[k];                                         /* no error: the feed-forward torque alone */
        else clipped += tk[k] == -8.0;                                               /* 20 x (-1 rad) + |tau_ff| < 12: clipped */
      }
      ticks += tick_status[b] != jstatus[(size_t)b * NROWS + first[b]];
    }
    printf("tick rc=%d mismatches=%d clipped=%d\n", rc, ticks, clipped);
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(joint); free(jstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (stamps ? 7 : (ticks || clipped != 12 ? 8 : 0));
}
