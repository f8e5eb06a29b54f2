/* The rollout through the feet from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_rolloutfeet_caller.py, tests/test_gpu_rollout_feet.py): the layout of QtosRolloutFeet by offsetof, what the argument
 * checks answer, and with a device one cold qtos_plan_batch of two robots on flat ground (a trot: two stance feet on most rows),
 * qtos_rollout_feet over 800 rows at 200 Hz without gains next to qtos_rollout on the same inputs (r and v must agree to the bit),
 * and with gains, with and without QTOS_FEET_LIMIT.
 * argv[1]: a QtosParams image written by the Python mirror.  Prints what the test compares; exit status 7 if a row of the run
 * without gains differs from qtos_rollout's in r or v, a time stamp differs, the limit's bit is set without the flag or the counters are
 * off.  Without a HIP device: the layout and what the argument checks answer, exit status 0. */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 200.0
#define NROWS 800

static const double INERTIA[3] = {0.00578574, 0.01938108, 0.02476124};

static void body(QtosRolloutFeet *r, const QtosParams *params, double gain) {
  int k;
  memset(r, 0, sizeof(*r));
  r->hz = HZ; r->substeps = 2; r->n_rows = NROWS; r->flags = QTOS_ROLLOUT_INIT;
  r->mass = params->mass; r->gravity = params->gravity; r->ff_scale = 1.0;
  for (k = 0; k < 3; ++k) {
    r->inertia_b[4 * k] = INERTIA[k]; r->inertia_b_inv[4 * k] = 1.0 / INERTIA[k];
    r->kp_lin[k] = 300.0 * gain; r->kd_lin[k] = 30.0 * gain; r->kp_ang[k] = 30.0 * gain; r->kd_ang[k] = 1.0 * gain;
  }
  r->arm = 0.2; r->damping = 1e-6; r->w_min = 0.01; r->mu = params->mu; r->f_max = params->f_max;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosRolloutFeet r, t;
  QtosRollout plain;
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB], state[NB * QTOS_ROLLOUT_STATE], state2[NB * QTOS_ROLLOUT_STATE];
  double worst_f = 0.0, worst_t = 0.0, worst_tilt = 0.0, nan_value;
  long long count[NB], count2[NB];
  double *nodes, *meas, *roll, *froll, *meas2, *roll2;
  int status[NB], iters[NB], word[NB], word2[NB], *rstatus, *rstatus2, rc, rc_dev, b, e, k, bad = 0, wrong = 0, two = 0, limited = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  body(&r, &params, 0.0);
  memset(count, 0, sizeof(count));
  memset(state, 0, sizeof(state));
  memset(word, 0, sizeof(word));
  printf("sizeof %d sizeof_rollout %d hz %d flags %d ff_scale %d push_ticks %d arm %d damping %d w_min %d mu %d f_max %d feet_flags %d\n",
         (int)sizeof(QtosRolloutFeet), (int)sizeof(QtosRollout), (int)offsetof(QtosRolloutFeet, hz), (int)offsetof(QtosRolloutFeet, flags),
         (int)offsetof(QtosRolloutFeet, ff_scale), (int)offsetof(QtosRolloutFeet, push_ticks), (int)offsetof(QtosRolloutFeet, arm), (int)offsetof(QtosRolloutFeet, damping),
         (int)offsetof(QtosRolloutFeet, w_min), (int)offsetof(QtosRolloutFeet, mu), (int)offsetof(QtosRolloutFeet, f_max),
         (int)offsetof(QtosRolloutFeet, feet_flags));
  printf("constants %d %d %d %d %d\n", QTOS_FEET_LIMIT, QTOS_ROLLOUT_FEET_COLS, QTOS_ROLLOUT_NO_STANCE, QTOS_ROLLOUT_TWO_STANCE, QTOS_ROLLOUT_LIMITED);
  rc = qtos_rollout_feet(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, NULL, status);
  rc_dev = qtos_rollout_feet_device(NULL, NB, &r, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, start, NULL, NULL, status, NULL);
  printf("rollout_feet_null=%d rollout_feet_device_null=%d\n", rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  meas = (double *)calloc((size_t)NB * NROWS * 18, sizeof(double));
  meas2 = (double *)calloc((size_t)NB * NROWS * 18, sizeof(double));
  roll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_COLS, sizeof(double));
  roll2 = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_COLS, sizeof(double));
  froll = (double *)calloc((size_t)NB * NROWS * QTOS_ROLLOUT_FEET_COLS, sizeof(double));
  rstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  rstatus2 = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !meas || !meas2 || !roll || !roll2 || !froll || !rstatus || !rstatus2) return 5;
  {  /* the argument checks that need a planner: -1 each, with a reason */
    int c[8];
    nan_value = 0.0;
    nan_value = nan_value / nan_value;
#define CALL(s) qtos_rollout_feet(p, NB, (s), nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, froll, rstatus)
    t = r; t.arm = 0.0; c[0] = CALL(&t);
    t = r; t.damping = 0.0; c[1] = CALL(&t);
    t = r; t.w_min = 0.0; c[2] = CALL(&t);
    t = r; t.w_min = 1.5; c[3] = CALL(&t);
    t = r; t.mu = -0.1; c[4] = CALL(&t);
    t = r; t.substeps = 0; c[5] = CALL(&t);
    c[6] = qtos_rollout_feet(p, NB, NULL, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state, count, word, meas, roll, froll, rstatus);
    t = r; t.mu = nan_value; c[7] = CALL(&t);
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
  if (!bad) {      /* no gains: r and v are qtos_rollout's, to the bit */
    memset(count2, 0, sizeof(count2));
    memset(state2, 0, sizeof(state2));
    memset(word2, 0, sizeof(word2));
    rc = CALL(&r);
    memcpy(&plain, &r, sizeof(plain));      /* the first sizeof(QtosRollout) bytes are a QtosRollout */
    rc_dev = qtos_rollout(p, NB, &plain, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, state2, count2, word2, meas2, roll2, rstatus2);
    bad |= rc != 0 || rc_dev != 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        const double *a = roll + i * QTOS_ROLLOUT_COLS, *c = roll2 + i * QTOS_ROLLOUT_COLS, *fr = froll + i * QTOS_ROLLOUT_FEET_COLS;
        wrong += memcmp(a, c, sizeof(double)) != 0 || memcmp(a + 1, c + 1, 3 * sizeof(double)) != 0 || memcmp(a + 7, c + 7, 3 * sizeof(double)) != 0;
        wrong += fr[0] != a[0] || fr[13] != 0.0 || fr[14] != 0.0 || fr[15] != 0.0;
        two += (rstatus[i] & QTOS_ROLLOUT_TWO_STANCE) != 0;
      }
    wrong += count[0] != NROWS || count[1] != NROWS || word[0] != word2[0] || word[1] != word2[1];
    printf("open rc=%d,%d mismatches=%d two_stance=%d\n", rc, rc_dev, wrong, two);
  }
  for (e = 0; e < 2 && !bad; ++e) {      /* with gains: what the feet do not deliver, without and with the limit */
    body(&t, &params, 1.0);
    t.feet_flags = e ? QTOS_FEET_LIMIT : 0;
    memset(count, 0, sizeof(count));
    memset(word, 0, sizeof(word));
    rc = CALL(&t);
    bad |= rc != 0;
    worst_f = worst_t = worst_tilt = 0.0;
    limited = 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        const double *fr = froll + i * QTOS_ROLLOUT_FEET_COLS;
        if (rstatus[i] & 3) continue;
        if (fr[13] > worst_f) worst_f = fr[13];
        if (fr[14] > worst_t) worst_t = fr[14];
        if (roll[i * QTOS_ROLLOUT_COLS + 18] > worst_tilt) worst_tilt = roll[i * QTOS_ROLLOUT_COLS + 18];
        limited += (rstatus[i] & QTOS_ROLLOUT_LIMITED) != 0;
      }
    wrong += e == 0 && limited != 0;
    printf("held limit=%d rc=%d miss_f=%.3e miss_t=%.3e tilt=%.3e limited=%d word=%d,%d mismatches=%d\n", e, rc, worst_f, worst_t, worst_tilt,
           limited, word[0], word[1], wrong);
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(meas); free(meas2); free(roll); free(roll2); free(froll); free(rstatus); free(rstatus2);
  qtos_planner_destroy(p);
  return bad ? 6 : (wrong ? 7 : 0);
}
