/* Plan, check, print from plain C99, host pointers only, no HIP and no torch on the caller's side (tests/test_plan_check_cpu.py,
 * tests/test_gpu_plan_check.py): one cold qtos_plan_batch of two robots on flat ground, qtos_sample_csv of its rows, qtos_plan_check
 * of the same rows with the table and the summary, and once more with the summary alone.
 * argv[1]: a QtosParams image written by the Python mirror; argv[2], if given: where the plans' node vectors go (NB x n_vars
 * doubles), so that the test checks the very same plans.  Prints what the tests compare, the summary as the bit patterns of
 * its maxima; exit status 7 if a time stamp of the check table differs from the CSV table's, 8 if the summary of the second
 * call differs from the first's.  Without a HIP device: the struct sizes and what the argument checks answer, exit status 0. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qtos_planner.h"

#define NB 2
#define HZ 100.0
#define NROWS 520

int main(int argc, char **argv) {
  static const double feet[QTOS_NEE][3] = {{0.21, 0.19, 0.0}, {0.21, -0.19, 0.0}, {-0.21, 0.19, 0.0}, {-0.21, -0.19, 0.0}};
  static const char *family[QTOS_CHECK_FAMILIES] = {"dyn_ang", "dyn_lin", "rom", "terrain", "force"};
  QtosParams params;
  QtosDims d;
  QtosPlanCheck c, t;
  QtosCheckRecord sum[NB * QTOS_CHECK_FAMILIES], again[NB * QTOS_CHECK_FAMILIES];
  QtosPlanner *p = NULL;
  double start[NB * QTOS_START_DOUBLES], goal[NB * 3], viol[NB], t0[NB];
  double *nodes, *rows, *check;
  int status[NB], iters[NB], rc, rc_dev, b, e, k, bad = 0, stamps = 0, differ = 0;
  FILE *f;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  memset(&c, 0, sizeof(c));
  c.hz = HZ; c.n_rows = NROWS;
  c.tol[0] = 1e-3; c.tol[1] = 1e-2; c.tol[2] = 1e-4; c.tol[3] = 1e-4; c.tol[4] = 1e-2;
  rc = qtos_plan_check(NULL, NB, &c, start, t0, NULL, NULL, NULL, NULL, start, sum);
  rc_dev = qtos_plan_check_device(NULL, NB, &c, start, t0, NULL, NULL, NULL, NULL, start, sum, NULL);
  printf("sizeof_plan_check=%d sizeof_check_record=%d check_null=%d check_device_null=%d\n", (int)sizeof(QtosPlanCheck),
         (int)sizeof(QtosCheckRecord), rc, rc_dev);
  rc = qtos_planner_create(&params, NB, 0, &p);
  if (rc == -2) {
    printf("create=%d: no HIP device, argument checks only\n", rc);
    return 0;
  }
  if (rc != 0 || qtos_planner_dims(p, &d) != 0) return 4;
  nodes = (double *)malloc(sizeof(double) * NB * (size_t)d.n_vars);
  rows = (double *)calloc((size_t)NB * NROWS * QTOS_CSV_COLS, sizeof(double));
  check = (double *)calloc((size_t)NB * NROWS * QTOS_CHECK_COLS, sizeof(double));
  if (!nodes || !rows || !check) return 5;
  {  /* the argument checks that need a planner: -1 each */
    int a[6];
    a[0] = qtos_plan_check(p, 0, &c, nodes, t0, NULL, NULL, NULL, NULL, check, sum);
    a[1] = qtos_plan_check(p, NB, &c, nodes, NULL, NULL, NULL, NULL, NULL, check, sum);
    a[2] = qtos_plan_check(p, NB, &c, nodes, t0, NULL, NULL, NULL, NULL, NULL, NULL);      /* both outputs NULL */
    t = c; t.n_rows = 0; a[3] = qtos_plan_check(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, check, sum);
    t = c; t.first_row = 1000001; a[4] = qtos_plan_check(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, check, sum);
    t = c; t.first_row = -1; a[5] = qtos_plan_check(p, NB, &t, nodes, t0, NULL, NULL, NULL, NULL, check, sum);
    printf("bad_args=%d,%d,%d,%d,%d,%d\n", a[0], a[1], a[2], a[3], a[4], a[5]);
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
    f = fopen(argv[2], "wb");
    bad |= !f || fwrite(nodes, sizeof(double), NB * (size_t)d.n_vars, f) != NB * (size_t)d.n_vars;
    if (f) fclose(f);
  }
  if (!bad) {
    rc = qtos_sample_csv(p, NB, nodes, t0, HZ, NROWS, rows);
    rc_dev = qtos_plan_check(p, NB, &c, nodes, t0, NULL, NULL, NULL, NULL, check, sum);
    bad |= rc != 0 || rc_dev != 0;
    for (b = 0; b < NB && !bad; ++b)
      for (k = 0; k < NROWS; ++k)
        stamps += check[((size_t)b * NROWS + k) * QTOS_CHECK_COLS] != rows[((size_t)b * NROWS + k) * QTOS_CSV_COLS];
    printf("sample rc=%d check rc=%d stamp_mismatches=%d\n", rc, rc_dev, stamps);
  }
  if (!bad) {                     /* the summary alone: the same records */
    rc = qtos_plan_check(p, NB, &c, nodes, t0, NULL, NULL, NULL, NULL, NULL, again);
    bad |= rc != 0;
    differ = !bad && memcmp(sum, again, sizeof(sum)) != 0;
    printf("summary_only rc=%d differ=%d\n", rc, differ);
  }
  for (b = 0; b < NB && !bad; ++b)
    for (k = 0; k < QTOS_CHECK_FAMILIES; ++k) {
      const QtosCheckRecord *r = sum + b * QTOS_CHECK_FAMILIES + k;
      unsigned long long bits;
      memcpy(&bits, &r->max, sizeof(bits));
      printf("window %d %s max=%.17g bits=%llx row=%lld count=%lld\n", b, family[k], r->max, bits, r->row, r->count);
    }
  if (bad) printf("error: %s\n", qtos_last_error(p));
  free(nodes); free(rows); free(check);
  qtos_planner_destroy(p);
  return bad ? 6 : (stamps ? 7 : (differ ? 8 : 0));
}
