/* The windows' robots as simulated rigid bodies from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_rollout_caller.py, tests/test_gpu_rollout.py): one cold qtos_plan_batch of two robots on flat ground, qtos_joint_rows
 * of its rows, qtos_rollout over the first 400 rows with QTOS_ROLLOUT_INIT and over the next 400 with the carried state, and
 * qtos_track of the rolled-out states.  The body has the URDF's diagonal inertia: the planner's reference-compat tensor is
 * indefinite, and a PD torque on it pushes the body away from its plan.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints what the test compares; exit status 7 if a time stamp of the
 * rollout table differs from the CSV table's, a measured row is not the rollout row's pose and the joint table's angles, or the
 * counters are off.  Without a HIP device: the struct size and what the argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 200.0
#define NROWS 800
#define HALF 400

static const double HIP[QTOS_NEE][3] = {{0.1946, 0.08750000000000001, 0.0}, {0.1946, -0.08750000000000001, 0.0}, {-0.1946, 0.08750000000000001, 0.0}, {-0.1946, -0.08750000000000001, 0.0}};
static const double INERTIA[3] = {0.00578574, 0.01938108, 0.02476124};

static void solo12(QtosJointRows *g, QtosTrack *w) {
  int e, k;      /* (the URDF's own digits: joints.SOLO12) */
  memset(g, 0, sizeof(*g));
  memset(w, 0, sizeof(*w));
  g->hz = w->hz = HZ; g->ee_shift = w->ee_shift = 0.015; g->l_upper = g->l_lower = w->l_upper = w->l_lower = 0.16; g->tau_max = 8.0;
  for (e = 0; e < QTOS_NEE; ++e) {
    for (k = 0; k < 3; ++k) g->hip[e][k] = w->hip[e][k] = HIP[e][k];
    g->lateral[e] = w->lateral[e] = (e % 2 ? -1.0 : 1.0) * (0.014 + 0.037450000000000004 + 0.008);
    g->knee_sign[e] = e < 2 ? -1.0 : 1.0;
  }
  for (k = 0; k < 12; ++k) { g->kp[k] = 20.0; g->kd[k] = 0.08; }
  w->delay = 0;
}

static void body(QtosRollout *r, const QtosParams *params) {
  int k;
  memset(r, 0, sizeof(*r));
  r->hz = HZ; r->substeps = 2; r->mass = params->mass; r->gravity = params->gravity; r->ff_scale = 1.0;
  for (k = 0; k < 3; ++k) {
    r->inertia_b[4 * k] = INERTIA[k]; r->inertia_b_inv[4 * k] = 1.0 / INERTIA[k];
    r->kp_lin[k] = 300.0; r->kd_lin[k] = 30.0; r->kp_ang[k] = 30.0; r->kd_ang[k] = 1.0;
  }
  r->dev_max = 0.5; r->tilt_max = 1.0;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosJointRows g;
  QtosTrack w;
  QtosRollout r, t;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB], total[NB * 2], state[NB * QTOS_ROLLOUT_STATE], worst = 0.0, worst_foot = 0.0;
  long long count[NB], tcount[NB * 2];
  double *nodes, *rows, *joint, *meas, *roll, *track;
  int status[NB], iters[NB], word[NB], *jstatus, *rstatus, *tstatus, rc, rc_dev, b, e, k, bad = 0, wrong = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  solo12(&g, &w);
  body(&r, &params);
  g.n_rows = w.n_rows = r.n_rows = NROWS;
  memset(count, 0, sizeof(count));
  memset(tcount, 0, sizeof(tcount));
  memset(total, 0, sizeof(total));
  memset(state, 0, sizeof(state));
  memset(word, 0, sizeof(word));
  rc = qtos_rollout(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, status);
  rc_dev = qtos_rollout_device(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, status, NULL);
  printf("sizeof_rollout=%d rollout_null=%d rollout_device_null=%d\n", (int)sizeof(QtosRollout), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  rows = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  joint = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  meas = (double *)calloc((size_t)NB * NROWS * 18, sizeof(double));
  roll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_COLS, sizeof(double));
  track = (double *)calloc((size_t)NB * NROWS * QTOS_TRACK_COLS, sizeof(double));
  jstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  rstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  tstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !rows || !joint || !meas || !roll || !track || !jstatus || !rstatus || !tstatus) return 5;
  {  /* the argument checks that need a planner: -1 each, with a reason */
    int c[8];
    t = r; t.substeps = 0; c[0] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    t = r; t.inertia_b[0] = t.inertia_b[4] = t.inertia_b[8] = 0.0;
    c[1] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    t = r; t.hz = 0.0; c[2] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    t = r; t.mass = -1.0; c[3] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    t = r; t.capacity = 8; c[4] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    c[5] = qtos_rollout(p, 0, &r, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    c[6] = qtos_rollout(p, NB, &r, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, count, word, meas, roll, rstatus);
    t = r; t.first_row = 1000001; c[7] = qtos_rollout(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, rstatus);
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d reason=%s\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], qtos_last_error(p));
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
  }
  if (!bad) {      /* two calls of 400 rows into the tables of 800: the per-window counts say how many, the second goes on from the first's state */
    int n[NB], at[NB];
    for (b = 0; b < NB; ++b) { n[b] = HALF; at[b] = 0; }
    t = r; t.flags = QTOS_ROLLOUT_INIT;
    rc = qtos_rollout(p, NB, &t, nodes, t0, at, n, NULL, joint, NULL, NULL, state, count, word, meas, roll, rstatus);
    bad |= rc != 0;
    wrong += count[0] != HALF || count[1] != HALF;
    if (!bad) {    /* the second half: a table of its own rows, behind the first */
      const size_t h18 = (size_t)HALF * 18, h20 = (size_t)HALF * QTOS_ROLLOUT_COLS, h37 = (size_t)HALF * QTOS_CSV_COLS;
      t = r; t.first_row = HALF; t.n_rows = HALF;
      for (b = 0; b < NB && !bad; ++b) {           /* (one window per call: its second half is contiguous in the table of 800) */
        const size_t o = (size_t)b * NROWS;
        rc = qtos_rollout(p, 1, &t, nodes + (size_t)b * d.n_vars, t0 + b, NULL, NULL, NULL, joint + o * QTOS_CSV_COLS + h37, NULL, NULL,
                          state + b * QTOS_ROLLOUT_STATE, count + b, word + b, meas + o * 18 + h18, roll + o * QTOS_ROLLOUT_COLS + h20,
                          rstatus + o + HALF);
        bad |= rc != 0;
      }
    }
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        const double *ro = roll + i * QTOS_ROLLOUT_COLS, *m = meas + i * 18;
        wrong += ro[0] != rows[i * QTOS_CSV_COLS];
        for (e = 0; e < 6; ++e) wrong += m[e] != ro[1 + e];
        for (e = 0; e < 12; ++e) wrong += m[6 + e] != joint[i * QTOS_CSV_COLS + 1 + e];
        if (ro[17] > worst) worst = ro[17];
      }
    wrong += count[0] != NROWS || count[1] != NROWS;
    printf("rollout rc=%d mismatches=%d worst_e=%.3e word=%d,%d\n", rc, wrong, worst, word[0], word[1]);
  }
  if (!bad) {
    rc = qtos_track(p, NB, &w, nodes, t0, NULL, NULL, NULL, meas, NULL, tcount, total, track, tstatus);
    bad |= rc != 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        if (track[i * QTOS_TRACK_COLS + 19] > worst) wrong += 1000;       /* k_track's CoM error is the rollout's |e| but for roundings */
        for (e = 20; e < 24; ++e) if (jstatus[i] == 0 && track[i * QTOS_TRACK_COLS + e] > worst_foot) worst_foot = track[i * QTOS_TRACK_COLS + e];
      }
    printf("track rc=%d worst_foot=%.3e recorded=%lld,%lld\n", rc, worst_foot, tcount[1], tcount[3]);
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(joint); free(meas); free(roll); free(track); free(jstatus); free(rstatus); free(tstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (wrong ? 7 : 0);
}
