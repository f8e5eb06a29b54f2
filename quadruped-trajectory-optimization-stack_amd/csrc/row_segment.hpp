// row_segment.hpp -- where rows first .. first + n - 1 of window b go: the one addressing of the window kernels' tables and rings.
//   table (capacity 0): row first + j is row j of the window's n_rows rows
//   ring  (capacity > 0): it is row (cursor[b] + j) mod capacity of the window's capacity rows, the floor modulus (a negative
//                         cursor lands in 0 .. capacity - 1)
// for j = 0 .. n - 1, n the window's count clamped to 0 .. rows_b (rows_b: n_rows or capacity), first clamped at 0.  Plain integer
// C++, no HIP types and no floating point: window_kernels.hpp and window_api.hpp compile it under hipcc, and
// tests/test_row_segment_cpu.py under g++, where it is held to the lines above over every small case.
#pragma once
#include <climits>
#include <cstddef>

#if defined(__HIPCC__)
#define QTOS_HD __host__ __device__
#else
#define QTOS_HD
#endif

namespace qtos {

// Rows a window's table or ring holds.
QTOS_HD inline long long segment_rows(long long capacity, int n_rows) { return capacity > 0 ? capacity : (long long)n_rows; }

struct RowSegment {   // the segment of one window: scalars only, so it lives in registers
  long long rows_b;   // rows of window b's table or ring
  long long n;        // the window's count, 0 .. rows_b
  long long pos;      // table or ring row of the segment's first row: 0 in a table, cursor mod capacity in a ring
  long long first;    // the plan row of the segment's first row, >= 0

  // capacity, n_rows, first_row: the scalars of the args struct; per_n, per_first: the per-window arrays, null for the scalars;
  // cursor: the rings' cursors, not read in table mode.
  QTOS_HD static RowSegment of(long long capacity, int n_rows, int first_row, const int *per_n, const int *per_first,
                               const long long *cursor, int b) {
    RowSegment G;
    G.rows_b = segment_rows(capacity, n_rows);
    const long long n = per_n ? per_n[b] : n_rows;
    G.n = n < 0 ? 0 : (n > G.rows_b ? G.rows_b : n);
    G.pos = 0;
    if (capacity > 0) {
      G.pos = cursor[b] % capacity;
      if (G.pos < 0) G.pos += capacity;
    }
    const long long first = per_first ? per_first[b] : first_row;
    G.first = first < 0 ? 0 : first;
    return G;
  }
  // Rows of the tile that starts at row j0 of the n, j0 < n.
  QTOS_HD int tile_rows(long long j0, int tile) const { return n - j0 < tile ? (int)(n - j0) : tile; }
  // Table or ring row of lane i of the tile at `base`, i < the tile's rows <= rows_b (base < rows_b: one subtraction wraps it).
  QTOS_HD long long tile_row(long long base, long long i) const { return base + i >= rows_b ? base + i - rows_b : base + i; }
  // Table or ring row of row j of the segment, j < rows_b: the base of the tile at j, and the single row of k_start_feedback.
  QTOS_HD long long row(long long j) const { return tile_row(pos, j); }
  // Element e of the tile at `base`, rows of `cols` elements, in the window's rows_b x cols elements: a tile that straddles the
  // wrap needs nothing else (e < the tile's rows x cols <= rows_b x cols: one subtraction).
  QTOS_HD long long flat(long long base, int cols, long long e) const {
    const long long all = rows_b * cols, o = base * cols + e;
    return o >= all ? o - all : o;
  }
  // The plan row of lane i of the tile at j0, as the int the sampler takes.
  QTOS_HD int plan_row(long long j0, long long i) const { return first + j0 + i > INT_MAX ? INT_MAX : (int)(first + j0 + i); }
};

// ---- the host side ----
// What is wrong with a segment's arguments, or null.  counted: the scalar n_rows is a count the kernel reads (k_stitch with
// per-window counts and k_start_feedback, which takes one row, do not read it as one).
inline const char *segment_check(long long capacity, int n_rows, int first_row, bool has_cursor, bool counted = true) {
  if (capacity < 0 || (capacity > 0 && !has_cursor)) return "capacity >= 0, and a ring needs its cursor";
  if ((counted && n_rows < 0) || (capacity == 0 && n_rows < 1)) return "n_rows >= 0, and a table has n_rows >= 1";
  if (first_row < 0 || first_row > 1000000) return "first_row is 0 .. 1000000";
  return nullptr;
}
// The most rows a window can have: the count where the host knows it, else what the table or ring holds.
inline long long most_rows(long long capacity, int n_rows, bool per_window) {
  return capacity > 0 ? (per_window || n_rows > capacity ? capacity : (long long)n_rows) : (long long)n_rows;
}
// Rows of B windows' tables or rings.
inline size_t segment_elems(int B, long long capacity, int n_rows) { return (size_t)B * (size_t)segment_rows(capacity, n_rows); }

}  // namespace qtos
