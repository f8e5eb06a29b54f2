/* Measured states and tracking errors of a plan from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_track_caller.py, tests/test_gpu_track.py): one cold qtos_plan_batch of two robots on flat ground, qtos_joint_rows of
 * its rows, a measured table built from the planned pose (qtos_sample_csv's columns 1 .. 6) and those joint angles, qtos_track of
 * it (table mode) and one tick: a row of its own per robot.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints what the test compares; exit status 7 if a time stamp of
 * the track table differs from the CSV table's or the counters are off, 8 if the tick is not the table's row.  Without a HIP
 * device: the struct size and what the argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 200.0
#define NROWS 1001
#define DELAY 3

static const double HIP[QTOS_NEE][3] = {{0.1946, 0.08750000000000001, 0.0}, {0.1946, -0.08750000000000001, 0.0}, {-0.1946, 0.08750000000000001, 0.0}, {-0.1946, -0.08750000000000001, 0.0}};

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
  w->delay = DELAY;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosJointRows g;
  QtosTrack w, t;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB], total[NB * 2], tick_total[NB * 2], tick_meas[NB * 18];
  double tick[NB * QTOS_TRACK_COLS], goal_x[NB], worst = 0.0;
  long long count[NB * 2], tick_count[NB * 2];
  double *nodes, *rows, *joint, *meas, *track;
  int status[NB], iters[NB], first[NB], tick_status[NB], *jstatus, *tstatus, rc, rc_dev, b, e, k, bad = 0, stamps = 0, ticks = 0, clean = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  solo12(&g, &w);
  g.n_rows = w.n_rows = NROWS;
  memset(count, 0, sizeof(count));
  memset(total, 0, sizeof(total));
  rc = qtos_track(NULL, NB, &w, start, t0, NULL, NULL, NULL, start, NULL, count, total, start, status);
  rc_dev = qtos_track_device(NULL, NB, &w, start, t0, NULL, NULL, NULL, start, NULL, count, total, start, status, NULL);
  printf("sizeof_track=%d track_null=%d track_device_null=%d\n", (int)sizeof(QtosTrack), rc, rc_dev);
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
  track = (double *)calloc((size_t)NB * NROWS * QTOS_TRACK_COLS, sizeof(double));
  jstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  tstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !rows || !joint || !meas || !track || !jstatus || !tstatus) return 5;
  {  /* the argument checks that need a planner: -1 each */
    long long cur[NB] = {0, 0};
    int c[9];
    c[0] = qtos_track(p, 0, &w, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    c[1] = qtos_track(p, NB, &w, nodes, t0, NULL, NULL, NULL, NULL, NULL, count, total, track, tstatus);
    t = w; t.capacity = 8; c[2] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);   /* a ring without cursor */
    t = w; t.capacity = -1; c[3] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, cur, meas, NULL, count, total, track, tstatus);
    t = w; t.n_rows = 0; c[4] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    t = w; t.first_row = 1000001; c[5] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    t = w; t.delay = -1; c[6] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    t = w; t.l_lower = 0.0; c[7] = qtos_track(p, NB, &t, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    c[8] = qtos_track(p, NB, &w, nodes, t0, NULL, NULL, NULL, meas, NULL, NULL, total, track, tstatus);
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d,%d\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]);
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
    /* the robot is where the plan wants it: the planned pose and the commanded angles */
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t r = (size_t)b * NROWS + k;
        for (e = 0; e < 6; ++e) meas[r * 18 + e] = rows[r * QTOS_CSV_COLS + 1 + e];
        for (e = 0; e < 12; ++e) meas[r * 18 + 6 + e] = joint[r * QTOS_CSV_COLS + 1 + e];
      }
  }
  if (!bad) {
    rc = qtos_track(p, NB, &w, nodes, t0, NULL, NULL, NULL, meas, NULL, count, total, track, tstatus);
    bad |= rc != 0;
    for (b = 0; b < NB && !bad; ++b) {
      for (k = 0; k < NROWS; ++k) {
        const size_t r = (size_t)b * NROWS + k;
        stamps += track[r * QTOS_TRACK_COLS] != rows[r * QTOS_CSV_COLS];
        stamps += (tstatus[r] & 1) != (k + 1 >= DELAY && k + 1 != DELAY + 1);
        if (jstatus[r] == 0) {       /* every leg within reach: the feet are where the plan has them */
          ++clean;
          for (e = 19; e < 24; ++e) if (track[r * QTOS_TRACK_COLS + e] > worst) worst = track[r * QTOS_TRACK_COLS + e];
        }
      }
      stamps += count[2 * b] != NROWS || count[2 * b + 1] != NROWS - DELAY;
      stamps += total[2 * b] != track[((size_t)b * NROWS + NROWS - 1) * QTOS_TRACK_COLS + 24];
      stamps += total[2 * b + 1] != track[((size_t)b * NROWS + NROWS - 1) * QTOS_TRACK_COLS + 25];
    }
    printf("track rc=%d mismatches=%d clean_rows=%d largest_error=%.3e\n", rc, stamps, clean, worst);
    printf("totals com=%.17g,%.17g feet=%.17g,%.17g recorded=%lld,%lld\n", total[0], total[2], total[1], total[3], count[1], count[3]);
  }
  if (!bad) {                     /* one tick: robot b at its row 100 + 150 b, with accumulators of its own; robot 1 has reached its goal */
    t = w; t.n_rows = 1; t.delay = 0;
    for (b = 0; b < NB; ++b) {
      first[b] = 100 + 150 * b;
      memcpy(tick_meas + 18 * b, meas + ((size_t)b * NROWS + first[b]) * 18, 18 * sizeof(double));
      tick_count[2 * b] = 40; tick_count[2 * b + 1] = 30;
      tick_total[2 * b] = 1.5; tick_total[2 * b + 1] = 2.5;
      goal_x[b] = tick_meas[18 * b] + (b ? -0.01 : 0.01);
    }
    rc = qtos_track(p, NB, &t, nodes, t0, first, NULL, NULL, tick_meas, goal_x, tick_count, tick_total, tick, tick_status);
    bad |= rc != 0;
    for (b = 0; b < NB && !bad; ++b) {
      const double *tr = track + ((size_t)b * NROWS + first[b]) * QTOS_TRACK_COLS, *tk = tick + b * QTOS_TRACK_COLS;
      for (k = 0; k < 24; ++k) ticks += tk[k] != tr[k];                              /* stamp, pose, errors: the table's */
      ticks += tk[24] != 1.5 + tr[19];
      ticks += tk[25] != 2.5 + tr[20] + tr[21] + tr[22] + tr[23];
      ticks += tick_total[2 * b] != tk[24] || tick_total[2 * b + 1] != tk[25];
      ticks += tick_count[2 * b] != 41 || tick_count[2 * b + 1] != 31;
      ticks += tick_status[b] != (b ? 3 : 1);
    }
    printf("tick rc=%d mismatches=%d\n", rc, ticks);
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(joint); free(meas); free(track); free(jstatus); free(tstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (stamps ? 7 : (ticks ? 8 : 0));
}
