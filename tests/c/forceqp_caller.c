/* The force fit inside the friction pyramid from plain C99, host pointers only, no HIP and no torch on the caller's side
 * (tests/test_forceqp_caller.py): one cold qtos_plan_batch of two robots on flat ground, qtos_sample_csv and qtos_joint_rows of
 * its rows, qtos_force_qp over them with the joint table (a force cap of 16 N, which the trot's two-stance rows exceed), and the
 * four records of every window.
 * argv[1]: a QtosParams image written by the Python mirror; argv[2] (optional): where the two plans' nodes are written.  Prints what
 * the tests compare; exit status 7 if a time stamp of the table differs from the CSV table's, the summary-only call answers other
 * records than the call with tables, or a row's smallest slack is not positive.  Without a HIP device: the struct size and what the
 * argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 100.0
#define NROWS 520

static const double HIP[QTOS_NEE][3] = {{0.1946, 0.08750000000000001, 0.0}, {0.1946, -0.08750000000000001, 0.0}, {-0.1946, 0.08750000000000001, 0.0}, {-0.1946, -0.08750000000000001, 0.0}};
static const char *FAMILY[QTOS_FIT_FAMILIES] = {"res_ang", "res_lin", "change", "limited"};

static void solo12(QtosJointRows *g, QtosForceQp *s) {
  int e, k;      /* (the URDF's own digits: joints.SOLO12) */
  memset(g, 0, sizeof(*g));
  memset(s, 0, sizeof(*s));
  g->hz = s->hz = HZ; g->ee_shift = s->ee_shift = 0.015; g->l_upper = g->l_lower = s->l_upper = s->l_lower = 0.16; g->tau_max = 8.0;
  for (e = 0; e < QTOS_NEE; ++e) {
    for (k = 0; k < 3; ++k) g->hip[e][k] = s->hip[e][k] = HIP[e][k];
    g->lateral[e] = s->lateral[e] = (e % 2 ? -1.0 : 1.0) * (0.014 + 0.037450000000000004 + 0.008);
    g->knee_sign[e] = s->knee_sign[e] = e < 2 ? -1.0 : 1.0;
  }
  for (k = 0; k < 12; ++k) { g->kp[k] = 20.0; g->kd[k] = 0.08; }
  s->arm = 0.2; s->damping = 1e-6; s->w_min = 0.01; s->excess_tol = 1e-2;
  s->mu = 0.5; s->f_max = 16.0; s->mu_end = 1e-6; s->act_tol = 1e-3; s->max_iter = QTOS_QP_MAX_ITER;
  s->tol[0] = 1e-3; s->tol[1] = 1e-2; s->tol[2] = 5.0; s->tol[3] = 1e-2;
}

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  QtosParams params;
  QtosDims d;
  QtosJointRows g;
  QtosForceQp s, t;
  QtosCheckRecord summary[NB * QTOS_FIT_FAMILIES], again[NB * QTOS_FIT_FAMILIES];
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB];
  double *nodes, *rows, *joint, *fit, *qrows;
  int status[NB], iters[NB], *jstatus, *fstatus, rc, rc_dev, b, e, k, f, bad = 0, wrong = 0, stamps = 0, two = 0, limited = 0, outside = 0;
  FILE *fh;
  if (argc < 2) return 2;
  fh = fopen(argv[1], "rb");
  if (!fh || fread(&params, sizeof(params), 1, fh) != 1) return 3;
  fclose(fh);
  solo12(&g, &s);
  g.n_rows = s.n_rows = NROWS;
  rc = qtos_force_qp(NULL, NB, &s, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, start, start, status, summary);
  rc_dev = qtos_force_qp_device(NULL, NB, &s, start, t0, NULL, NULL, NULL, NULL, NULL, NULL, start, start, status, summary, NULL);
  printf("sizeof_force_qp=%d sizeof_check_record=%d qp_null=%d qp_device_null=%d\n", (int)sizeof(QtosForceQp), (int)sizeof(QtosCheckRecord),
         rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  rows = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  joint = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  fit = (double *)calloc((size_t)NB * NROWS * QTOS_FIT_COLS, sizeof(double));
  qrows = (double *)calloc((size_t)NB * NROWS * QTOS_QP_COLS, sizeof(double));
  jstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  fstatus = (int *)calloc((size_t)NB * NROWS, sizeof(int));
  if (!nodes || !rows || !joint || !fit || !qrows || !jstatus || !fstatus) return 5;
  {  /* the argument checks that need a planner: -1 each, with a reason */
    int c[8];
    t = s; t.mu = 0.0; c[0] = qtos_force_qp(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
    t = s; t.f_max = -1.0; c[1] = qtos_force_qp(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
    t = s; t.mu_end = 0.0; c[2] = qtos_force_qp(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
    t = s; t.max_iter = 26; c[3] = qtos_force_qp(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
    c[4] = qtos_force_qp(p, 0, &s, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
    c[5] = qtos_force_qp(p, NB, &s, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    c[6] = qtos_force_qp(p, NB, &s, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, qrows, NULL, summary);
    t = s; t.arm = 0.0; c[7] = qtos_force_qp(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, fit, qrows, fstatus, summary);
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
  if (!bad && argc > 2) {
    fh = fopen(argv[2], "wb");
    if (!fh || fwrite(nodes, sizeof(double), NB * (size_t)d.n_vars, fh) != NB * (size_t)d.n_vars) return 3;
    fclose(fh);
  }
  if (!bad) {
    rc = qtos_sample_csv(p, NB, nodes, t0, HZ, NROWS, rows);
    rc_dev = qtos_joint_rows(p, NB, &g, nodes, t0, NULL, NULL, NULL, NULL, NULL, joint, jstatus);
    bad |= rc != 0 || rc_dev != 0;
  }
  if (!bad) {
    rc = qtos_force_qp(p, NB, &s, nodes, t0, NULL, NULL, NULL, NULL, joint, NULL, fit, qrows, fstatus, summary);
    rc_dev = qtos_force_qp(p, NB, &s, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, again);     /* the records alone */
    bad |= rc != 0 || rc_dev != 0;
  }
  if (!bad) {
    for (b = 0; b < NB; ++b)
      for (k = 0; k < NROWS; ++k) {
        const size_t i = (size_t)b * NROWS + k;
        const double *c = rows + i * QTOS_CSV_COLS, *r = fit + i * QTOS_FIT_COLS;
        stamps += r[0] != c[0];
        two += (fstatus[i] & QTOS_QP_TWO_STANCE) != 0;
        limited += (fstatus[i] & QTOS_QP_LIMITED) != 0;
        outside += !(qrows[i * QTOS_QP_COLS + 3] > 0.0);
      }
    wrong += stamps + outside + (memcmp(summary, again, sizeof(summary)) != 0);
    printf("qp rc=%d stamp_mismatches=%d differ=%d two_stance_rows=%d limited_rows=%d outside=%d\n", rc, stamps,
           memcmp(summary, again, sizeof(summary)) != 0, two, limited, outside);
    for (b = 0; b < NB; ++b)
      for (f = 0; f < QTOS_FIT_FAMILIES; ++f) {
        const QtosCheckRecord *q = summary + b * QTOS_FIT_FAMILIES + f;
        unsigned long long word;
        memcpy(&word, &q->max, sizeof(word));
        printf("window %d %s max=%.6e bits=%llx row=%lld count=%lld\n", b, FAMILY[f], q->max, word, q->row, q->count);
      }
  }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(joint); free(fit); free(qrows); free(jstatus); free(fstatus);
  qtos_planner_destroy(p);
  return bad ? 6 : (wrong ? 7 : 0);
}
