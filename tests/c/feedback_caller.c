/* A replan that starts from the measured state, from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_feedback_caller.py, tests/test_gpu_feedback.py): one cold qtos_plan_batch of two robots on flat ground,
 * qtos_handover, a measured state for the row in front of the hand-over row -- the planned pose (qtos_sample_csv's columns 1 ..
 * 6) shifted by DRIFT and the commanded joint angles (qtos_joint_rows) --, qtos_start_feedback of it (table mode) and the next
 * qtos_plan_batch from the corrected start.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints what the test compares; exit status 7 if the corrected start
 * is not the hand-over's + DRIFT in x and y of the CoM and the feet.  Without a HIP device: the struct size and what the argument
 * checks answer, exit status 0. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 1000.0

static const double HIP[QTOS_NEE][3] = {{0.1946, 0.08750000000000001, 0.0}, {0.1946, -0.08750000000000001, 0.0}, {-0.1946, 0.08750000000000001, 0.0}, {-0.1946, -0.08750000000000001, 0.0}};
static const double NOMINAL[QTOS_NEE][3] = {{0.20, 0.17, -0.26}, {0.20, -0.17, -0.26}, {-0.20, 0.17, -0.26}, {-0.20, -0.17, -0.26}};
static const double DRIFT[2] = {0.010, -0.005};

static void solo12(QtosJointRows *g, QtosFeedback *w) {
  int e, k;      /* (the URDF's own digits: joints.SOLO12; the box: PlannerConfig's) */
  memset(g, 0, sizeof(*g));
  memset(w, 0, sizeof(*w));
  g->hz = w->hz = HZ; g->ee_shift = w->ee_shift = 0.015; g->l_upper = g->l_lower = w->l_upper = w->l_lower = 0.16; g->tau_max = 8.0;
  for (e = 0; e < QTOS_NEE; ++e) {
    for (k = 0; k < 3; ++k) { g->hip[e][k] = w->hip[e][k] = HIP[e][k]; w->nominal[e][k] = NOMINAL[e][k]; }
    g->lateral[e] = w->lateral[e] = (e % 2 ? -1.0 : 1.0) * (0.014 + 0.037450000000000004 + 0.008);
    g->knee_sign[e] = e < 2 ? -1.0 : 1.0;
  }
  for (k = 0; k < 12; ++k) { g->kp[k] = 20.0; g->kd[k] = 0.08; }
  w->gain_pos = w->gain_ang = w->gain_foot = 1.0;
  w->max_pos = 0.05; w->max_ang = 0.2; w->max_foot = 0.05;
  w->max_deviation[0] = w->max_deviation[1] = 0.07; w->max_deviation[2] = 0.09;
  w->rom_tol = 1e-6; w->snap_tol = 0.02;
  w->flags = QTOS_FEEDBACK_SNAP;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosHandover h;
  QtosJointRows g;
  QtosFeedback w, t;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], handed[NB * QTOS_START_DOUBLES], goal[NB * 3], goal_step[NB * 3], offset[NB], viol[NB], t0[NB];
  double err[NB * 18], worst = 0.0;
  double *nodes, *rows = NULL, *joint = NULL, *meas = NULL;
  int row[NB], status[NB], iters[NB], fstatus[NB], *jstatus = NULL, rc, rc_dev, b, e, k, n, bad = 0, miss = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  solo12(&g, &w);
  w.n_rows = 1;
  memset(&h, 0, sizeof(h));
  h.advance = 2.5; h.search = 0.4; h.hz = HZ; h.rule = 0;
  rc = qtos_start_feedback(NULL, NB, &w, start, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
  rc_dev = qtos_start_feedback_device(NULL, NB, &w, start, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus, NULL);
  printf("sizeof_feedback=%d feedback_null=%d feedback_device_null=%d\n", (int)sizeof(QtosFeedback), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  if (!nodes) return 5;
  {  /* the argument checks that need a planner: -1 each */
    int c[8];
    c[0] = qtos_start_feedback(p, 0, &w, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    c[1] = qtos_start_feedback(p, NB, &w, nodes, t0, NULL, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    t = w; t.capacity = 8; c[2] = qtos_start_feedback(p, NB, &t, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);   /* a ring without cursor */
    t = w; t.n_rows = 0; c[3] = qtos_start_feedback(p, NB, &t, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    t = w; t.latency = -1.0; c[4] = qtos_start_feedback(p, NB, &t, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    t = w; t.gain_foot = 1.5; c[5] = qtos_start_feedback(p, NB, &t, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    t = w; t.max_ang = 0.0; c[6] = qtos_start_feedback(p, NB, &t, nodes, t0, row, NULL, start, NULL, start, NULL, NULL, err, fstatus);
    c[7] = qtos_start_feedback(p, NB, &w, nodes, t0, row, NULL, start, NULL, start, goal_step, NULL, err, fstatus);                       /* goal_step without goal */
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
  }
  memset(start, 0, sizeof(start));
  for (b = 0; b < NB; ++b) {      /* at rest in nominal stance, 0.1 m apart; every plan's goal 0.09 m per second of horizon ahead */
    double *s = start + b * QTOS_START_DOUBLES;
    s[0] = 0.1 * b; s[2] = 0.24;
    for (e = 0; e < QTOS_NEE; ++e)
      for (k = 0; k < 3; ++k) s[6 + 3 * e + k] = feet[e][k] + (k == 0 ? s[0] : 0.0);
    goal_step[3 * b] = 0.09 * d.duration; goal_step[3 * b + 1] = goal_step[3 * b + 2] = 0.0;
    goal[3 * b] = s[0] + goal_step[3 * b]; goal[3 * b + 1] = 0.0; goal[3 * b + 2] = 0.24;
    t0[b] = 10.0 * b;
  }
  rc = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
  printf("plan rc=%d status=%d,%d\n", rc, status[0], status[1]);
  bad |= rc != 0;
  if (!bad) {
    rc = qtos_handover(p, NB, &h, nodes, goal_step, start, goal, offset, row);
    bad |= rc != 0;
    memcpy(handed, start, sizeof(start));
  }
  if (!bad) {                     /* the measured rows: a table up to the later hand-over row; only the row in front of each is filled */
    n = row[0] > row[1] ? row[0] : row[1];
    rows = (double *)calloc((size_t)NB * n * QTOS_CSV_COLS, sizeof(double));
    joint = (double *)calloc((size_t)NB * n * QTOS_CSV_COLS, sizeof(double));
    meas = (double *)calloc((size_t)NB * n * 18, sizeof(double));
    jstatus = (int *)calloc((size_t)NB * n, sizeof(int));
    if (!rows || !joint || !meas || !jstatus || row[0] < 1 || row[1] < 1) return 5;
    g.n_rows = w.n_rows = n;
    rc = qtos_sample_csv(p, NB, nodes, t0, HZ, n, rows);
    rc_dev = qtos_joint_rows(p, NB, &g, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    bad |= rc != 0 || rc_dev != 0;
    for (b = 0; b < NB && !bad; ++b) {
      const size_t r = (size_t)b * n + (row[b] - 1);
      for (e = 0; e < 6; ++e) meas[r * 18 + e] = rows[r * QTOS_CSV_COLS + 1 + e] + (e < 2 ? DRIFT[e] : 0.0);
      for (e = 0; e < 12; ++e) meas[r * 18 + 6 + e] = joint[r * QTOS_CSV_COLS + 1 + e];
    }
  }
  if (!bad) {
    rc = qtos_start_feedback(p, NB, &w, nodes, t0, row, NULL, meas, NULL, start, goal_step, goal, err, fstatus);
    bad |= rc != 0;
    for (b = 0; b < NB && !bad; ++b) {
      const double *s = start + b * QTOS_START_DOUBLES, *o = handed + b * QTOS_START_DOUBLES;
      for (k = 0; k < 2; ++k) {
        double m = fabs(s[k] - (o[k] + DRIFT[k]));
        if (m > worst) worst = m;
        for (e = 0; e < QTOS_NEE; ++e) {
          m = fabs(s[6 + 3 * e + k] - (o[6 + 3 * e + k] + DRIFT[k]));
          if (m > worst) worst = m;
        }
        miss += goal[3 * b + k] != s[k] + goal_step[3 * b + k];
      }
      for (k = 18; k < QTOS_START_DOUBLES; ++k) miss += s[k] != o[k];      /* the velocities stay the plan's */
    }
    miss += !(worst < 1e-12);
    printf("feedback rc=%d status=%d,%d largest_miss=%.3e mismatches=%d\n", rc, fstatus[0], fstatus[1], worst, miss);
  }
  if (!bad) {
    rc = qtos_plan_batch(p, NB, start, goal, NULL, NULL, nodes, status, iters, viol);
    printf("replan rc=%d status=%d,%d\n", rc, status[0], status[1]);
    bad |= rc != 0;
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(joint); free(meas); free(jstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (miss ? 7 : 0);
}
