// row_segment_host.cpp -- csrc/row_segment.hpp under g++ (test infrastructure, compiled by tests/test_row_segment_cpu.py): every
// member is called the way the window kernels call it, over arrays of cases, and nothing is computed here but by the header.
#include "row_segment.hpp"

using qtos::RowSegment;

extern "C" {

// N cases.  Per case: capacity, n_rows, first_row (the scalars), per_n and per_first (used where has_per is not 0), cursor, the
// tile size.  seg [N, 4]: rows_b, n, pos, first.  row, plan [N, pitch]: the table or ring row and the plan row of row j of the
// segment, written tile by tile as a kernel walks them.  flat [N, pitch * cols]: the offset of element c of row j.  single
// [N, pitch]: row(j) for every j < rows_b.  Entries that no lane of the case writes stay as they come.  Returns the cases
// whose rows_b does not fit the pitch (0 in a test that sized its arrays).
int rs_cases(int N, const long long *capacity, const int *n_rows, const int *first_row, const int *has_per, const int *per_n,
             const int *per_first, const long long *cursor, const int *tile, int cols, int pitch, long long *seg, long long *row,
             long long *plan, long long *flat, long long *single) {
  int bad = 0;
  for (int c = 0; c < N; ++c) {
    // (one window: the per-window arrays and the cursor are read at b = 0)
    const RowSegment G = RowSegment::of(capacity[c], n_rows[c], first_row[c], has_per[c] ? per_n + c : nullptr,
                                        has_per[c] ? per_first + c : nullptr, cursor + c, 0);
    seg[4 * c] = G.rows_b; seg[4 * c + 1] = G.n; seg[4 * c + 2] = G.pos; seg[4 * c + 3] = G.first;
    if (G.rows_b > pitch || G.n > pitch) { ++bad; continue; }
    for (long long j0 = 0; j0 < G.n; j0 += tile[c]) {
      const int m = G.tile_rows(j0, tile[c]);
      const long long base = G.row(j0);
      for (int i = 0; i < m; ++i) {
        row[(long long)c * pitch + j0 + i] = G.tile_row(base, i);
        plan[(long long)c * pitch + j0 + i] = G.plan_row(j0, i);
      }
      for (int e = 0; e < m * cols; ++e) flat[((long long)c * pitch + j0) * cols + e] = G.flat(base, cols, e);
    }
    for (long long j = 0; j < G.rows_b; ++j) single[(long long)c * pitch + j] = G.row(j);
  }
  return bad;
}

// segment_check's reason (null: the arguments are fine), most_rows and segment_elems.
const char *rs_check(long long capacity, int n_rows, int first_row, int has_cursor, int counted) {
  return qtos::segment_check(capacity, n_rows, first_row, has_cursor != 0, counted != 0);
}
long long rs_most_rows(long long capacity, int n_rows, int per_window) { return qtos::most_rows(capacity, n_rows, per_window != 0); }
unsigned long long rs_elems(int B, long long capacity, int n_rows) { return qtos::segment_elems(B, capacity, n_rows); }
}
