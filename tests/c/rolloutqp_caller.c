/* The rollout with the force QP from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_rolloutqp_caller.py): the layout of QtosRolloutQp by offsetof next to QtosRolloutFeet's, what the argument checks
 * answer, and with a device one cold qtos_plan_batch of two robots on flat ground (a trot), qtos_joint_rows of their plans, and the
 * closed loop over 800 rows at 200 Hz with gains and tight limits (mu 0.5, a cap of 16 N), once with qtos_rollout_feet's clip
 * (QTOS_FEET_LIMIT) and once with qtos_rollout_qp.
 * argv[1]: a QtosParams image, argv[2]: a QtosJointRows image, both written by the Python mirror.  Prints what the test compares;
 * exit status 7 if a time stamp differs, an alive stance force of the QP lies outside the limits, a measured joint angle is not the
 * joint row's, or the counters are off.  Without a HIP device: the layout and what the argument checks answer, exit status 0. */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 200.0
#define NROWS 800
#define MU 0.5
#define FMAX 16.0

static const double INERTIA[3] = {0.00578574, 0.01938108, 0.02476124};

static void body(QtosRolloutQp *r, const QtosParams *params) {
  int k;
  memset(r, 0, sizeof(*r));
  r->hz = HZ; r->substeps = 2; r->n_rows = NROWS; r->flags = QTOS_ROLLOUT_INIT;
  r->mass = params->mass; r->gravity = params->gravity; r->ff_scale = 1.0;
  for (k = 0; k < 3; ++k) {
    r->inertia_b[4 * k] = INERTIA[k]; r->inertia_b_inv[4 * k] = 1.0 / INERTIA[k];
    r->kp_lin[k] = 300.0; r->kd_lin[k] = 30.0; r->kp_ang[k] = 30.0; r->kd_ang[k] = 1.0;
  }
  r->dev_max = 0.5; r->tilt_max = 1.0;
  r->arm = 0.2; r->damping = 1e-2; r->w_min = 0.01; r->mu = MU; r->f_max = FMAX;
  r->mu_end = 1e-6; r->act_tol = 1e-3; r->max_iter = QTOS_QP_MAX_ITER;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosJointRows jp;
  QtosDims d;
  QtosRolloutQp r, t;
  QtosRolloutFeet clip;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB], state[NB * QTOS_ROLLOUT_STATE];
  double worst_f, worst_t, worst_tilt, nan_value;
  long long count[NB];
  double *nodes, *meas, *roll, *froll, *qroll, *joint;
  int status[NB], iters[NB], word[NB], *rstatus, *jstatus, rc, rc_dev, b, e, k, bad = 0, wrong = 0, limited, capped, frozen, most;
  FILE *f;
  if (argc < 3) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  f = fopen(argv[2], "rb");
  if (!f || fread(&jp, sizeof(jp), 1, f) != 1) return 3;
  fclose(f);
  body(&r, &params);
  memset(count, 0, sizeof(count));
  memset(state, 0, sizeof(state));
  memset(word, 0, sizeof(word));
  printf("sizeof %d sizeof_feet %d arm %d,%d f_max %d,%d feet_flags %d,%d mu_end %d act_tol %d max_iter %d\n", (int)sizeof(QtosRolloutQp),
         (int)sizeof(QtosRolloutFeet), (int)offsetof(QtosRolloutQp, arm), (int)offsetof(QtosRolloutFeet, arm), (int)offsetof(QtosRolloutQp, f_max),
         (int)offsetof(QtosRolloutFeet, f_max), (int)offsetof(QtosRolloutQp, feet_flags), (int)offsetof(QtosRolloutFeet, feet_flags),
         (int)offsetof(QtosRolloutQp, mu_end), (int)offsetof(QtosRolloutQp, act_tol), (int)offsetof(QtosRolloutQp, max_iter));
  printf("constants %d %d %d\n", QTOS_ROLLOUT_QP_COLS, QTOS_ROLLOUT_CAP, QTOS_ROLLOUT_LIMITED);
  rc = qtos_rollout_qp(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, NULL, NULL, status);
  rc_dev = qtos_rollout_qp_device(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, NULL, NULL, status, NULL);
  printf("rollout_qp_null=%d rollout_qp_device_null=%d\n", rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  meas = (double *)calloc((size_t)NB * NROWS * 18, sizeof(double));
  roll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_COLS, sizeof(double));
  froll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_FEET_COLS, sizeof(double));
  qroll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_QP_COLS, sizeof(double));
  joint = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  rstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  jstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !meas || !roll || !froll || !qroll || !joint || !rstatus || !jstatus) return 5;
  {  /* the argument checks that need a planner: -1 each, with a reason */
    int c[10];
    nan_value = 0.0;
    nan_value = nan_value / nan_value;
#define CALL(s) qtos_rollout_qp(p, NB, (s), nodes, t0, NULL, NULL, NULL, joint, NULL, NULL, state, count, word, meas, roll, froll, qroll, rstatus)
    t = r; t.arm = 0.0; c[0] = CALL(&t);
    t = r; t.substeps = 0; c[1] = CALL(&t);
    c[2] = qtos_rollout_qp(p, NB, NULL, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, froll, qroll, rstatus);
    t = r; t.mu = 0.0; c[3] = CALL(&t);
    t = r; t.f_max = 0.0; c[4] = CALL(&t);
    t = r; t.mu_end = 0.0; c[5] = CALL(&t);
    t = r; t.max_iter = 0; c[6] = CALL(&t);
    t = r; t.max_iter = QTOS_QP_MAX_ITER + 1; c[7] = CALL(&t);
    t = r; t.mu_end = nan_value; c[8] = CALL(&t);
    t = r; t.act_tol = nan_value; c[9] = CALL(&t);
    printf("bad_args=%d,%d,%d,%d,%d,%d,%d,%d,%d,%d reason=%s\n", c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8], c[9], qtos_last_error(p));
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
  if (!bad) {      /* the joint rows of the plans: the measured joint angles of the rollout */
    jp.hz = HZ; jp.first_row = 0; jp.n_rows = NROWS; jp.capacity = 0;
    rc = qtos_joint_rows(p, NB, &jp, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    printf("joint rc=%d\n", rc);
    bad |= rc != 0;
  }
  for (e = 0; e < 2 && !bad; ++e) {      /* the closed loop with the clip, then with the QP */
    memset(count, 0, sizeof(count));
    memset(word, 0, sizeof(word));
    if (e == 0) {
      memcpy(&clip, &r, sizeof(clip));      /* QtosRolloutQp begins with QtosRolloutFeet's fields at its offsets */
      clip.feet_flags = QTOS_FEET_LIMIT;
      rc = qtos_rollout_feet(p, NB, &clip, nodes, t0, NULL, NULL, NULL, joint, NULL, NULL, state, count, word, meas, roll, froll, rstatus);
    } else {
      rc = CALL(&r);
    }
    bad |= rc != 0;
    worst_f = worst_t = worst_tilt = 0.0;
    limited = capped = frozen = most = 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        const double *fr = froll + i * QTOS_ROLLOUT_FEET_COLS, *q = qroll + i * QTOS_ROLLOUT_QP_COLS, *a = roll + i * QTOS_ROLLOUT_COLS;
        int c;
        wrong += fr[0] != a[0] || a[0] != joint[i * QTOS_CSV_COLS];
        wrong += memcmp(meas + i * 18 + 6, joint + i * QTOS_CSV_COLS + 1, 12 * sizeof(double)) != 0;
        if (rstatus[i] & 3) { ++frozen; continue; }
        if (fr[13] > worst_f) worst_f = fr[13];
        if (fr[14] > worst_t) worst_t = fr[14];
        if (a[18] > worst_tilt) worst_tilt = a[18];
        limited += (rstatus[i] & QTOS_ROLLOUT_LIMITED) != 0;
        capped += (rstatus[i] & QTOS_ROLLOUT_CAP) != 0;
        if (e == 1) {
          if ((int)q[0] > most) most = (int)q[0];
          for (c = 0; c < QTOS_NEE; ++c) {      /* a stance force of the QP is strictly inside; a swing foot's is the plan's: 0 but for roundings */
            const double *fc = fr + 1 + 3 * c;
            if (fc[0] < 1e-12 && fc[0] > -1e-12 && fc[1] < 1e-12 && fc[1] > -1e-12 && fc[2] < 1e-12 && fc[2] > -1e-12) continue;
            wrong += !(fc[2] > 0.0 && fc[2] < FMAX && fc[0] < MU * fc[2] && -fc[0] < MU * fc[2] && fc[1] < MU * fc[2] && -fc[1] < MU * fc[2]);
          }
        }
      }
    wrong += count[0] != NROWS || count[1] != NROWS || (e == 0 && capped != 0);
    printf("held qp=%d rc=%d miss_f=%.3e miss_t=%.3e tilt=%.3e limited=%d cap=%d frozen=%d most_steps=%d word=%d,%d mismatches=%d\n", e, rc, worst_f,
           worst_t, worst_tilt, limited, capped, frozen, most, word[0], word[1], wrong);
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(meas); free(roll); free(froll); free(qroll); free(joint); free(rstatus); free(jstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (wrong ? 7 : 0);
}
