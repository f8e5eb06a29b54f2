/* The create-time KKT self-test from C99 (tests/test_selftest_cpu.py): the struct the Python mirror reads, and what the entry
 * points answer on a machine without a HIP device.  argv[1]: a QtosParams image written by the Python mirror. */
#include <stdio.h>
#include <string.h>

#include "qtos_planner.h"

int main(int argc, char **argv) {
  QtosParams params;
  QtosSelftest t, tried[3];
  QtosPlanner *p = (QtosPlanner *)&params; /* (any non-null value: the call must reset it) */
  FILE *f;
  int n_tried = 7, rc_null, rc_null_out, rc_checked, rc_bad, rules[3], fronts[3], stages[3], n_cand;
  if (argc < 2) return 2;
  f = fopen(argv[1], "rb");
  if (!f || fread(&params, sizeof(params), 1, f) != 1) return 3;
  fclose(f);
  memset(&t, 0, sizeof(t));
  rc_null = qtos_planner_selftest(NULL, 0ull, 0.0, &t);
  rc_null_out = qtos_planner_selftest(NULL, 0ull, 0.0, NULL);
  rc_checked = qtos_planner_create_checked(&params, 2, 0, 0, 0.0, &p, tried, 3, &n_tried);
  printf("sizeof_selftest=%d sizeof_params=%d sizeof_dims=%d selftest_null=%d selftest_null_out=%d checked=%d out_null=%d n_tried=%d\n",
         (int)sizeof(QtosSelftest), (int)sizeof(QtosParams), (int)sizeof(QtosDims), rc_null, rc_null_out, rc_checked, p == NULL, n_tried);
  rc_bad = qtos_planner_create_checked(NULL, 2, 0, 0, 0.0, &p, tried, 3, &n_tried);
  n_cand = qtos_analyze_candidates(&params, 0, rules, fronts, stages, 3);
  printf("checked_null_params=%d n_candidates=%d first_rule=%d first_front=%d first_stages=%d bits=%llu\n", rc_bad, n_cand, rules[0], fronts[0],
         stages[0], qtos_selftest_bits(1ull, 0, 2, 3ull));
  if (p) qtos_planner_destroy(p);
  return 0;
}
