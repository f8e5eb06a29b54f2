// window_kernels.hpp -- gfx950 device code around the solve: the sampler and the kernels of the receding loop (the "windows").
// They read plans through SamplePlan; of the solver's kernels (kernels.hpp) they use the terrain look-up (terrain_at) and, in
// k_plan_check, the pieces of the Newton-Euler and force rows (dyn_angular, rotation, trig_of, terrain_basis, wg_reduce).
//
//   k_sample        : 1 kHz spline sampling into the 37-column CSV row layout
//   k_handover      : start, goal and clock offset of the next window from the plan that is running
//   k_stitch        : the rows a window executed, appended to its trajectory ring
//   k_joint_rows    : joint commands of the windows' plans (leg IK and motor law)
//   k_track         : measured states and tracking errors of the windows
//   k_start_feedback: the next plan's start from the measured state
//   k_plan_check    : what the windows' plans violate between their knots
//   k_rollout       : the windows' robots as simulated rigid bodies (the measured states k_track reads)
//   k_force_fit     : the rows' contact forces fitted to the planned motion (k_plan_check's pieces and a 6 x 6 solve per row)
//   k_force_qp      : that fit inside the friction pyramid (k_force_fit's pieces and an interior-point solve per limited row)
//   k_path_goal     : goals of the windows from their global paths
//   k_path_plan     : the global paths (A* and spines)
//   k_probe*        : the probe and the stamp of the windows' heightfields
//   k_terrain_env   : the randomised terrains of the windows
//
// The argument checks and launches are in window_api.hpp.
#pragma once
#include "kernels.hpp"
#include "row_segment.hpp"

namespace qtos {

// =================================================================================================
// CSV sampling: row layout of QTOS/utils.py:107-148.  Spline lookup tables are built on the host.
struct SampleSpline {
  int n_polys;
  const double *tend;  // cumulative end time of each polynomial; behind them, tend[n_polys + k]: what the float64 start
                       // tend[k] - dur[k] of polynomial k is off its exact start by (sample_spline<true>)
  const double *dur;
  const int *idx;      // (n_polys+1) x 6
};
struct SamplePlan {
  SampleSpline lin, ang, eem[NEE], eef[NEE];
  int n_vars;
  double T;
};

// EXACT_START: the local time is taken from the polynomial's exact start (the float64 start and its correction word), so it
// carries the rounding of t alone and not that of the cumulative table as well.  The first derivative of a force polynomial of
// a short stance (12 ms on a 1 s horizon) has a slope of 6 / T^2 = 4e4 per second at its nodes, times node values tens of
// newtons apart: the table's half ulp of t was 2e-10 .. 5e-10 N/s in k_shift_warm's force derivatives (tests/test_gpu_splines.py).
// The rows of k_sample, k_stitch and k_handover hold values and base velocities only and keep the plain form, bit for bit.
template <bool EXACT_START = false>
__device__ inline void sample_spline(const SampleSpline &S, const double *x, double t, int deriv, double out[3]) {
  // first polynomial whose end time >= t - eps (towr spline.cc GetSegmentID)
  int lo = 0, hi = S.n_polys - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.tend[mid] >= t - 1e-10) hi = mid; else lo = mid + 1;
  }
  const int k = lo;
  const double T = S.dur[k];
  double tau = t - (S.tend[k] - T);
  if (EXACT_START) tau -= S.tend[S.n_polys + k];
  double w[4];
  const double T2 = T * T, T3 = T2 * T, t2 = tau * tau, t3 = t2 * tau;
  if (deriv == 0) {
    w[0] = 1 - 3 * t2 / T2 + 2 * t3 / T3; w[1] = tau - 2 * t2 / T + t3 / T2;
    w[2] = 3 * t2 / T2 - 2 * t3 / T3; w[3] = -t2 / T + t3 / T2;
  } else {
    w[0] = -6 * tau / T2 + 6 * t2 / T3; w[1] = 1 - 4 * tau / T + 3 * t2 / T2;
    w[2] = 6 * tau / T2 - 6 * t2 / T3; w[3] = -2 * tau / T + 3 * t2 / T2;
  }
  for (int d = 0; d < 3; ++d) {
    double acc = 0;
    for (int a = 0; a < 4; ++a) {
      const int v = S.idx[(k + (a >> 1)) * 6 + (a & 1) * 3 + d];
      if (v >= 0) acc += w[a] * x[v];
    }
    out[d] = acc;
  }
}

// Columns 1 .. 24 of a CSV row (the state a plan starts from, QTOS/combiner.py:263-274) at plan time t: k_sample's rows and
// the one row k_handover evaluates per window go through these lines, so the two agree to the bit.
__device__ inline void sample_row_state(const SamplePlan &S, const double *x, double t, double *row) {
  sample_spline(S.lin, x, t, 0, row + 1);
  sample_spline(S.ang, x, t, 0, row + 4);
  for (int e = 0; e < NEE; ++e) sample_spline(S.eem[e], x, t, 0, row + 7 + 3 * e);
  sample_spline(S.lin, x, t, 1, row + 19);
  sample_spline(S.ang, x, t, 1, row + 22);
}

// Row k of a plan's CSV (QTOS/utils.py:107-148) but its forces: the time stamp t0 + k / hz in column 0 and the state in columns
// 1 .. 24 at plan time min(k / hz, T).  Returns that plan time: the caller evaluates the four force splines of columns 25 .. 36
// at it, in a loop of its own over S.eef -- with that loop in here k_sample, which takes the tables by value, loads all of
// them into scalar registers at its start (93 instead of 35) and is no longer the code it was.  k_sample's table and the rows
// k_stitch appends go through these lines and the same line for the forces, so the two agree to the bit.
__device__ inline double sample_row_state_at(const SamplePlan &S, const double *x, double t0, int k, double hz, double *row) {
  double t = k / hz;
  if (t > S.T) t = S.T;
  row[0] = t0 + k / hz;
  sample_row_state(S, x, t, row);
  return t;
}

__global__ __launch_bounds__(256) void k_sample(SamplePlan S, const double *nodes, const double *t0, double hz,
                                                int n_rows, double *rows, int B) {
  const int b = blockIdx.y;
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B || k >= n_rows) return;
  const double *x = nodes + (size_t)b * S.n_vars;
  double row[QTOS_CSV_COLS];
  const double t = sample_row_state_at(S, x, t0[b], k, hz, row);
  for (int e = 0; e < NEE; ++e) sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
  double *out = rows + ((size_t)b * n_rows + k) * QTOS_CSV_COLS;
  for (int i = 0; i < QTOS_CSV_COLS; ++i) out[i] = row[i];
}

// Hand-over of a receding-horizon replan (qtos_handover*; QTOS/combiner.py:78-92, 245-296): one workgroup per window picks
// the row of the window's newest plan the next plan starts from -- the first of the candidate rows k0 .. k0 + n_search with
// all four feet in contact, k0 where none passes -- and evaluates that one row: no table of rows is written.  Lanes stride
// over the candidates and evaluate only what the rule reads (z of the four force splines / of the four foot splines, the
// very expressions of k_sample: the rule sees the numbers a sampled table would hold); the winning row's columns 1 .. 24
// come from k_sample's own evaluator.  No scratch: the sampling tables come through a pointer (by value, as k_sample
// takes them, the ten splines and these arguments do not fit the scalar registers), and the heights are read with constant
// indices (a loop over an array in the kernel arguments copies it to scratch, see k_shift_warm).
struct HandoverArgs {   // QtosHandover as the kernel reads it (window_api.hpp handover_args)
  double hz, x_lo, x_hi;
  double h6[8];         // rint(height * 1e6); NaN (equal to nothing) beyond n_heights
  int rule, zero_filter, turn;
  int k0, n_search;     // candidate rows k0 .. k0 + n_search
};

__device__ inline bool handover_contact(const SamplePlan &S, const HandoverArgs &H, const double *x, double t) {
  bool all = true;
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    double o3[3];
    if (H.rule == 0) {   // (uniform over the workgroup)
      sample_spline(S.eef[e], x, t, 0, o3);
      all = all && o3[2] > 0;
    } else {
      sample_spline(S.eem[e], x, t, 0, o3);
      const double z6 = rint(o3[2] * 1e6);
      all = all && (z6 == H.h6[0] || z6 == H.h6[1] || z6 == H.h6[2] || z6 == H.h6[3] || z6 == H.h6[4] || z6 == H.h6[5] ||
                    z6 == H.h6[6] || z6 == H.h6[7]);
    }
  }
  return all;
}

__global__ __launch_bounds__(512) void k_handover(const SamplePlan *Sd, HandoverArgs H, const double *nodes, double *goal_step,
                                                  double *start_out, double *goal_out, double *offset_out, int *row_out, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  __shared__ int first;
  const SamplePlan &S = *Sd;
  const double *x = nodes + (size_t)b * S.n_vars;
  if (threadIdx.x == 0) first = INT_MAX;
  __syncthreads();
  for (int k = H.k0 + threadIdx.x; k <= H.k0 + H.n_search; k += blockDim.x) {   // (ascending per lane: its first hit is its smallest)
    double t = k / H.hz;
    if (t > S.T) t = S.T;
    if (handover_contact(S, H, x, t)) { atomicMin(&first, k); break; }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const int k = first == INT_MAX ? H.k0 : first;
  double t = k / H.hz;
  if (t > S.T) t = S.T;
  double row[1 + QTOS_START_DOUBLES];
  sample_row_state(S, x, t, row);
  double *st = start_out + (size_t)b * QTOS_START_DOUBLES;
#pragma unroll
  for (int i = 0; i < QTOS_START_DOUBLES; ++i) {
    if (H.zero_filter && fabs(row[1 + i]) < 1e-4) row[1 + i] = 0.0;     // QTOS/utils.py zero_filter
    st[i] = row[1 + i];
  }
  offset_out[b] = (double)k / H.hz;
  if (row_out) row_out[b] = k;
  if (goal_step) {
    double *gs = goal_step + (size_t)b * 3;
    double gx = gs[0];
    if (H.turn) {   // a window past an end of its heightfield turns round
      const double sgn = row[1] > H.x_hi ? -1.0 : (row[1] < H.x_lo ? 1.0 : (gx > 0 ? 1.0 : (gx < 0 ? -1.0 : 0.0)));
      gx = sgn * fabs(gx);
      gs[0] = gx;
    }
    goal_out[(size_t)b * 3 + 0] = row[1] + gx;
    goal_out[(size_t)b * 3 + 1] = row[2] + gs[1];
  }
}

// Stitching of receding windows (qtos_stitch*; Combiner.combine, QTOS/combiner.py:125-135, 298-312): one workgroup per window
// appends rows first_row .. first_row + n - 1 of the window's plan -- the segment that was executed before the next plan took
// over -- to the window's ring of CSV rows, then moves the window's cursor and clock on.  One workgroup per window, so the
// cursor and the clock are updated in place: every lane reads them before the barrier, lane 0 writes them at the end.
// A lane evaluates one row of a tile with k_sample's evaluator (sample_row_state_at) and puts it into LDS; the tile then goes out
// flat, consecutive lanes on consecutive doubles of the ring (k_sample's row per lane is 37 stores at a stride of 296 bytes;
// this kernel is bound by its stores).  The LDS image keeps the rows' pitch of 37 doubles = 74 dwords: the 16 lanes of a
// ds_write_b64 group land on banks 10 l mod 32 and the bank after each, all 32 distinct, and the flat read-back is
// consecutive.  Element e of a tile goes to double (base * 37 + e) mod (capacity * 37) of the ring, base the ring row of
// the tile's first row: a tile that straddles the wrap needs nothing else.  That is RowSegment's rule (row_segment.hpp), spelled
// out here, the ring alone: through RowSegment the 256 x 2500-row launch measured 0.3 - 1.5 % slower than these lines, with the
// segment formed in front of the first barrier or behind it ("Row segments").  No scratch: the tables come through a
// pointer and the row array is indexed with constants only (see k_handover).
constexpr int STITCH_TILE = 512;   // rows per tile = lanes per workgroup: 512 x 37 x 8 = 151 552 bytes of LDS, one workgroup per CU
struct StitchArgs {                // QtosStitch as the kernel reads it (window_api.hpp stitch_args)
  double hz;
  long long capacity;
  int first_row, n_rows, advance_clock;
};

// A tile of m rows of COLS doubles, in LDS at that pitch, goes out flat to the window's rows `dst` from row `base` on:
// consecutive lanes on consecutive doubles, `lanes` of them.
template <int COLS>
__device__ inline void segment_tile_out(const RowSegment &G, long long base, int m, const double *tile, double *dst, int lanes) {
  for (int e = threadIdx.x; e < m * COLS; e += lanes) dst[G.flat(base, COLS, e)] = tile[e];
}

__global__ __launch_bounds__(STITCH_TILE) void k_stitch(const SamplePlan *Sd, StitchArgs A, const double *nodes, const int *n_rows,
                                                        double *t0, double *traj, long long *cursor, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  __shared__ double tile[STITCH_TILE * QTOS_CSV_COLS];
  const SamplePlan &S = *Sd;
  const double *x = nodes + (size_t)b * S.n_vars;
  const long long cur = cursor[b];
  const double t0b = t0[b];
  long long n = n_rows ? n_rows[b] : A.n_rows;
  n = n < 0 ? 0 : (n > A.capacity ? A.capacity : n);
  __syncthreads();                                       // (every lane holds the cursor and the clock: lane 0 may write them)
  double *ring = traj + (size_t)b * (size_t)A.capacity * QTOS_CSV_COLS;
  const long long ring_doubles = A.capacity * QTOS_CSV_COLS;
  long long pos = cur % A.capacity;                      // ring row of the segment's first row
  if (pos < 0) pos += A.capacity;
  for (long long j0 = 0; j0 < n; j0 += STITCH_TILE) {    // (n is uniform over the workgroup: so are the barriers)
    const int m = n - j0 < STITCH_TILE ? (int)(n - j0) : STITCH_TILE;
    if ((int)threadIdx.x < m) {
      const long long k = (long long)A.first_row + j0 + threadIdx.x;
      double row[QTOS_CSV_COLS];
      const double t = sample_row_state_at(S, x, t0b, k > INT_MAX ? INT_MAX : (int)k, A.hz, row);
      for (int e = 0; e < NEE; ++e) sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
      double *dst = tile + threadIdx.x * QTOS_CSV_COLS;
#pragma unroll
      for (int i = 0; i < QTOS_CSV_COLS; ++i) dst[i] = row[i];
    }
    __syncthreads();
    long long base = pos + j0;                           // (pos < capacity and j0 < n <= capacity: one subtraction wraps it)
    if (base >= A.capacity) base -= A.capacity;
    base *= QTOS_CSV_COLS;
    for (int e = threadIdx.x; e < m * QTOS_CSV_COLS; e += STITCH_TILE) {
      long long o = base + e;                            // (m <= capacity: o < 2 ring_doubles)
      if (o >= ring_doubles) o -= ring_doubles;
      ring[o] = tile[e];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    cursor[b] = cur + n;
    if (A.advance_clock) t0[b] = t0b + (double)n / A.hz;
  }
}

// Joint commands of the windows' plans (qtos_joint_rows*; scripts/run.py:184-200, QTOS/robot/robot.py control_multi): per CSV row
// the feet in the base frame of the planned pose (towr_transform, QTOS/utils.py:412-436), the closed-form inverse kinematics
// of the SOLO12 leg (HAA about x, HFE and KFE about y; the reference asks PyBullet), the joint rates qdot = J^-1 v_b, the
// feed-forward torques -J^T R^T f and the motor law (MotorModel.convert_to_torque_ff).  The statement of the rule, with its
// derivation, is joints.py.  A lane evaluates one row: its time stamp and Cartesian state with k_sample's evaluator
// (sample_row_state_at and the line for the forces: qtos_sample_csv's numbers to the bit), the four foot splines once more
// with deriv = 1, then the chain for four legs, written into the row's place in an LDS tile as it is computed; the tile goes
// out flat, consecutive lanes on consecutive doubles, as k_stitch's (whose pitch of 37 doubles it keeps).  The tile has one
// row per lane of the workgroup: 512, or one wave where no window has more rows than that (the 1 kHz tick).
// Both addressing modes of RowSegment (row_segment.hpp): a B x n_rows x 37 table or a B x capacity x 37 ring; cursor and t0 are
// only read, so the grid runs over tiles and windows in both modes, and in front of k_stitch on one stream the joint ring is
// filled row for row with the CSV ring.  The status goes out one int per lane, to the same row of a B x (n_rows | capacity) array.
// No atomics and no scratch: the tables come through a pointer (see k_handover), the arrays of the arguments are read with
// constant indices only (joint_leg is a template over the leg), and the math library's sincos, which returns the cosine
// through a pointer, is not used.
struct JointArgs {   // QtosJointRows as the kernel reads it (window_api.hpp joint_args)
  double hz, ee_shift, l_upper, l_lower, tau_max;
  double hip[NEE][3], lateral[NEE], knee_sign[NEE], kp[3 * NEE], kd[3 * NEE];
  long long capacity;
  int first_row, n_rows, flags;
};
constexpr int JOINT_TILE = 512;   // rows per tile = lanes per workgroup (see STITCH_TILE); JOINT_TICK where a window has one wave of rows
constexpr int JOINT_TICK = 64;    // at the most: 18 944 bytes of LDS, several workgroups per CU

// MotorModel.convert_to_torque_ff as joints.motor_torque states it: every operation one rounded IEEE operation in numpy's
// order (the library is built with the compiler's default, which fuses a * b + c: switched off here), np.clip's comparisons.
__device__ inline double joint_motor(double kp, double kd, double q, double qd, double tff, double tau_max, bool pd, double qm,
                                     double qdm) {
#pragma clang fp contract(off)
  double tau = tff;
  if (pd) {
    const double a = kp * (q - qm), b = kd * (qd - qdm);
    tau = (a + b) + tff;
  }
  if (tau_max > 0) tau = tau < -tau_max ? -tau_max : (tau > tau_max ? tau_max : tau);
  return tau;
}

// R = Rz(yaw) Ry(pitch) Rx(roll) of a row's Euler angles (row-major) and the angular velocity in the base frame from its Euler
// rates.  Like joint_leg without contraction: which product of a sum the compiler fuses is its choice per instantiation, and
// the 64-lane tick then differed from the 512-lane table in the last bit of qdot; one rounded operation each, they agree.
__device__ inline void joint_pose(const double *row, double R[9], double wb[3]) {
#pragma clang fp contract(off)
  const double sa = sin(row[4]), ca = cos(row[4]), sb = sin(row[5]), cb = cos(row[5]), sc = sin(row[6]), cc = cos(row[6]);
  R[0] = cc * cb; R[1] = cc * sb * sa - sc * ca; R[2] = cc * sb * ca + sc * sa;
  R[3] = sc * cb; R[4] = sc * sb * sa + cc * ca; R[5] = sc * sb * ca - cc * sa;
  R[6] = -sb; R[7] = cb * sa; R[8] = cb * ca;
  wb[0] = row[22] - row[24] * sb; wb[1] = row[23] * ca + row[24] * cb * sa; wb[2] = row[24] * cb * ca - row[23] * sa;
}

// Leg E of a row: R the rotation of the planned pose (row-major), wb the angular velocity in the base frame, fv the foot's
// velocity.  Writes q, qdot and tau of the leg's three joints to dst (the row's place in the tile); returns the status bits.
template <int E>
__device__ inline int joint_leg(const JointArgs &A, const double *row, const double R[9], const double wb[3], const double fv[3],
                                const double *q_mes, const double *qd_mes, double *dst) {
#pragma clang fp contract(off)
  const double d = A.lateral[E], lu = A.l_upper, ll = A.l_lower;
  const double *pf = row + 7 + 3 * E, *f = row + 25 + 3 * E;
  const double dx = pf[0] - row[1], dy = pf[1] - row[2], dz = pf[2] - row[3];
  const double ux = fv[0] - row[19], uy = fv[1] - row[20], uz = fv[2] - row[21];
  // r_b = R^T (foot - com); v_b = R^T (foot_vel - com_vel) - wb x r_b; p_b = r_b + (0, 0, ee_shift)
  const double bx = R[0] * dx + R[3] * dy + R[6] * dz, by = R[1] * dx + R[4] * dy + R[7] * dz, bz = R[2] * dx + R[5] * dy + R[8] * dz;
  const double vx = R[0] * ux + R[3] * uy + R[6] * uz - (wb[1] * bz - wb[2] * by);
  const double vy = R[1] * ux + R[4] * uy + R[7] * uz - (wb[2] * bx - wb[0] * bz);
  const double vz = R[2] * ux + R[5] * uy + R[8] * uz - (wb[0] * by - wb[1] * bx);
  const double rx = bx - A.hip[E][0], ry = by - A.hip[E][1], rz = bz + A.ee_shift - A.hip[E][2];
  // inverse kinematics (joints.leg_ik)
  // (the two clips are comparisons, as feedback_clip: a NaN stays a NaN where fmax and fmin would drop it; a target with a
  // non-finite component gives NaN angles and rates, never a finite number)
  const bool finite = isfinite(rx) && isfinite(ry) && isfinite(rz);
  const double h2 = ry * ry + rz * rz - d * d;
  const double h2c = h2 < 0 ? 0.0 : h2;
  double h = sqrt(h2c);
  const double c3 = (rx * rx + h2c - lu * lu - ll * ll) / (2 * lu * ll);
  const int status = (c3 > 1 ? 1 : 0) | (c3 < -1 ? 1 << 4 : 0) | (h2 < 0 ? 1 << 8 : 0);
  double q3 = finite ? A.knee_sign[E] * acos(c3 < -1 ? -1.0 : (c3 > 1 ? 1.0 : c3)) : NAN;
  if (finite && c3 < -0.5) {
    // the fold side (joints.leg_ik): c3 + 1 and h^2 are small differences there, so h^2 is formed as (r_y - d)(r_y + d) + r_z^2
    // and the knee from the half angle, both numerators from rho^2 directly; the status bits stay the comparisons above
    const double hf2 = (ry - d) * (ry + d) + rz * rz;
    h = h2 < 0 ? 0.0 : sqrt(hf2 < 0 ? 0.0 : hf2);
    const double rho2 = rx * rx + h * h;
    const double a = ((lu + ll) * (lu + ll) - rho2) / (2 * lu * ll), b = (rho2 - (lu - ll) * (lu - ll)) / (2 * lu * ll);
    q3 = A.knee_sign[E] * (2 * atan2(sqrt(a < 0 ? 0.0 : a), sqrt(c3 < -1 || b < 0 ? 0.0 : b)));
  }
  const double q1 = finite ? atan2(ry * h + rz * d, ry * d - rz * h) : NAN;
  const double s3 = sin(q3), c3c = cos(q3);
  const double q2 = finite ? atan2(-rx, h) - atan2(ll * s3, lu + ll * c3c) : NAN;
  // the chain at q (joints._hip_frame): the foot at (x, d, -hh) in the hip frame
  const double s1 = sin(q1), c1 = cos(q1), s2 = sin(q2), c2 = cos(q2), s23 = sin(q2 + q3), c23 = cos(q2 + q3);
  const double x = -lu * s2 - ll * s23, hh = lu * c2 + ll * c23, ls = ll * s23, lc = ll * c23;
  // joint rates (joints.joint_rates): zero for a leg with a status bit
  double qd1 = finite ? 0 : NAN, qd2 = qd1, qd3 = qd1;
  if (!status) {
    const double wy = c1 * vy + s1 * vz, wz = c1 * vz - s1 * vy, det = -(lu * ll * s3);
    qd1 = wy / hh;
    const double r2 = wz - d * qd1;
    qd2 = (vx * ls + lc * r2) / det;
    qd3 = (x * vx - hh * r2) / det;
  }
  // feed-forward torques (joints.feed_forward)
  double t1 = 0, t2 = 0, t3 = 0;
  if (!(A.flags & 1)) {
    const double fx = R[0] * f[0] + R[3] * f[1] + R[6] * f[2], fy = R[1] * f[0] + R[4] * f[1] + R[7] * f[2],
                 fz = R[2] * f[0] + R[5] * f[1] + R[8] * f[2];
    const double gy = c1 * fy + s1 * fz, gz = c1 * fz - s1 * fy;
    t1 = -(hh * gy + d * gz); t2 = hh * fx + x * gz; t3 = lc * fx - ls * gz;
  }
  const bool pd = q_mes != nullptr;
  const double m1 = pd ? q_mes[3 * E] : 0, m2 = pd ? q_mes[3 * E + 1] : 0, m3 = pd ? q_mes[3 * E + 2] : 0;
  const double n1 = pd ? qd_mes[3 * E] : 0, n2 = pd ? qd_mes[3 * E + 1] : 0, n3 = pd ? qd_mes[3 * E + 2] : 0;
  dst[1 + 3 * E] = q1; dst[2 + 3 * E] = q2; dst[3 + 3 * E] = q3;
  dst[13 + 3 * E] = qd1; dst[14 + 3 * E] = qd2; dst[15 + 3 * E] = qd3;
  dst[25 + 3 * E] = joint_motor(A.kp[3 * E], A.kd[3 * E], q1, qd1, t1, A.tau_max, pd, m1, n1);
  dst[26 + 3 * E] = joint_motor(A.kp[3 * E + 1], A.kd[3 * E + 1], q2, qd2, t2, A.tau_max, pd, m2, n2);
  dst[27 + 3 * E] = joint_motor(A.kp[3 * E + 2], A.kd[3 * E + 2], q3, qd3, t3, A.tau_max, pd, m3, n3);
  // NONFINITE: one of the leg's nine numbers q, qdot, tau_ff is not finite (a non-finite input; a division by a determinant
  // that is exactly zero)
  const bool all_finite = isfinite(q1) && isfinite(q2) && isfinite(q3) && isfinite(qd1) && isfinite(qd2) && isfinite(qd3) &&
                          isfinite(t1) && isfinite(t2) && isfinite(t3);
  return (status | (all_finite ? 0 : 1 << 12)) << E;
}

template <int TILE>
__global__ __launch_bounds__(TILE) void k_joint_rows(const SamplePlan *Sd, JointArgs A, const double *nodes, const double *t0,
                                                     const int *first_row, const int *n_rows, const long long *cursor,
                                                     const double *q_mes, const double *qd_mes, double *out, int *status_out, int B) {
  __shared__ double joint_tile[TILE * QTOS_CSV_COLS];
  const int b = blockIdx.y;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long j0 = (long long)blockIdx.x * blockDim.x;                        // first row of this tile, of the n rows
  if (j0 >= G.n) return;                                                           // (uniform over the workgroup)
  const int m = G.tile_rows(j0, (int)blockDim.x);
  const long long base = G.row(j0);
  if ((int)threadIdx.x < m) {
    const double *x = nodes + (size_t)b * S.n_vars;
    double row[QTOS_CSV_COLS];
    const double t = sample_row_state_at(S, x, t0[b], G.plan_row(j0, threadIdx.x), A.hz, row);
    for (int e = 0; e < NEE; ++e) sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
    double fv[NEE][3];
    for (int e = 0; e < NEE; ++e) sample_spline(S.eem[e], x, t, 1, fv[e]);
    double R[9], wb[3];
    joint_pose(row, R, wb);
    const double *qm = q_mes ? q_mes + (size_t)b * 3 * NEE : nullptr, *qdm = q_mes ? qd_mes + (size_t)b * 3 * NEE : nullptr;
    double *dst = joint_tile + threadIdx.x * QTOS_CSV_COLS;
    dst[0] = row[0];
    int st = joint_leg<0>(A, row, R, wb, fv[0], qm, qdm, dst);
    st |= joint_leg<1>(A, row, R, wb, fv[1], qm, qdm, dst);
    st |= joint_leg<2>(A, row, R, wb, fv[2], qm, qdm, dst);
    st |= joint_leg<3>(A, row, R, wb, fv[3], qm, qdm, dst);
    status_out[(size_t)b * (size_t)G.rows_b + G.tile_row(base, threadIdx.x)] = st;
  }
  __syncthreads();
  segment_tile_out<QTOS_CSV_COLS>(G, base, m, joint_tile, out + (size_t)b * (size_t)G.rows_b * QTOS_CSV_COLS, blockDim.x);
}

// Measured states and tracking errors of the windows (qtos_track*; scripts/run.py:244-273, QTOS/tracking.py Tracking.update /
// _update, QTOS/robot/robot.py traj_vec): the counterpart of k_joint_rows for what comes back from the robot.  Per CSV row the
// measured base pose and joint angles become the reference's traj_vec (CoM, Euler angles, the four feet in the world by the
// leg's closed-form forward kinematics, joints.leg_fk), the five Euclidean errors against the plan's own row and the two
// running totals.  The statement of the rule is tracking.py.  The totals are sequential sums by definition, so one workgroup
// owns one window and walks its tiles in order.  Per tile: (A) a lane takes a row -- time stamp and planned positions with
// k_sample's evaluator (sample_row_state_at: qtos_sample_csv's numbers to the bit), R from the measured pose, four legs through
// a template over the leg, and the 24 values and five errors into the row's place of an LDS tile; (B) behind a barrier lane 0
// runs the CoM chain over the tile's rows and the first lane of the second wave the feet chain (lane 0 again where the
// workgroup is one wave), each from the total it carries in a register from the previous tile, into columns 24 and 25; (C) the
// tile goes out flat, consecutive lanes on consecutive doubles, the pitch of 26 doubles kept (RowSegment's addressing: table or
// ring, cursor and t0 only read).  The status is one int per lane.  The owners of the chains write count and total back with
// plain stores behind the last tile; every lane has read them in front of the first barrier.  No atomics, no scratch (constant
// indices only, see k_joint_rows), no sincos.
struct TrackArgs {   // QtosTrack as the kernel reads it (window_api.hpp track_args)
  double hz, ee_shift, l_upper, l_lower;
  double hip[NEE][3], lateral[NEE];
  long long capacity;
  int first_row, n_rows, delay, flags;
};
constexpr int TRACK_COLS = 26;
constexpr int TRACK_TILE = 512;   // rows per tile = lanes per workgroup: 512 x 26 x 8 = 106 496 bytes of LDS, one workgroup per CU
constexpr int TRACK_TICK = 64;    // one wave where no window has more rows (the tick): 13 312 bytes

// R (row-major) of the measured pose and the Euler columns.  Euler mode (m[3 .. 5] roll, pitch, yaw): R = Rz Ry Rx as
// joint_pose forms it, the angles copied through.  Quaternion mode (m[3 .. 6] = x, y, z, w): divided by its norm, R directly,
// roll = atan2(R21, R22), pitch = asin(clip(-R20)), yaw = atan2(R10, R00); returns 4 (GIMBAL) where the clip acts.  Without
// contraction, as joint_pose: one rounded operation each, in tracking.py's order.
__device__ inline int track_pose(const double *m, bool quat, double R[9], double *euler) {
#pragma clang fp contract(off)
  if (!quat) {
    const double sa = sin(m[3]), ca = cos(m[3]), sb = sin(m[4]), cb = cos(m[4]), sc = sin(m[5]), cc = cos(m[5]);
    R[0] = cc * cb; R[1] = cc * sb * sa - sc * ca; R[2] = cc * sb * ca + sc * sa;
    R[3] = sc * cb; R[4] = sc * sb * sa + cc * ca; R[5] = sc * sb * ca - cc * sa;
    R[6] = -sb; R[7] = cb * sa; R[8] = cb * ca;
    euler[0] = m[3]; euler[1] = m[4]; euler[2] = m[5];
    return 0;
  }
  double x = m[3], y = m[4], z = m[5], w = m[6];
  const double n = sqrt(((x * x + y * y) + z * z) + w * w);
  x = x / n; y = y / n; z = z / n; w = w / n;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
  euler[0] = atan2(R[7], R[8]);
  const double sp = -R[6];
  euler[1] = asin(sp < -1 ? -1.0 : (sp > 1 ? 1.0 : sp));                             // (comparisons: a NaN stays a NaN, without the bit)
  euler[2] = atan2(R[3], R[0]);
  return fabs(R[6]) >= 1 ? 4 : 0;
}

// |a - b| of two points: sqrt((d0 d0 + d1 d1) + d2 d2), one rounded operation after the other (tracking.errors).
__device__ inline double track_norm(const double *a, const double *b) {
#pragma clang fp contract(off)
  const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2];
  return sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// Foot E of a measured row in the world: com + R (leg_fk(E, q) - (0, 0, ee_shift)), q the leg's three measured angles
// (joints.leg_fk: hip + Rx(q1) (x, d, -h)).  Writes the foot to dst[7 + 3 E ..] and its error against the planned foot to
// dst[20 + E] (dst: the row's place in the tile).
template <int E>
__device__ inline void track_leg(const TrackArgs &A, const double *row, const double *com, const double R[9], const double *q,
                                 double *dst) {
#pragma clang fp contract(off)
  const double d = A.lateral[E], lu = A.l_upper, ll = A.l_lower;
  const double q1 = q[3 * E], q2 = q[3 * E + 1], q3 = q[3 * E + 2];
  const double s1 = sin(q1), c1 = cos(q1), s2 = sin(q2), c2 = cos(q2), s23 = sin(q2 + q3), c23 = cos(q2 + q3);
  const double x = -lu * s2 - ll * s23, h = lu * c2 + ll * c23;
  const double px = A.hip[E][0] + x, py = A.hip[E][1] + c1 * d + s1 * h, pz = (A.hip[E][2] + s1 * d - c1 * h) - A.ee_shift;
  double foot[3];
  foot[0] = com[0] + ((R[0] * px + R[1] * py) + R[2] * pz);
  foot[1] = com[1] + ((R[3] * px + R[4] * py) + R[5] * pz);
  foot[2] = com[2] + ((R[6] * px + R[7] * py) + R[8] * pz);
  dst[7 + 3 * E] = foot[0]; dst[8 + 3 * E] = foot[1]; dst[9 + 3 * E] = foot[2];
  dst[20 + E] = track_norm(row + 7 + 3 * E, foot);
}

// Whether the 1-based call c of a window is recorded (tracking.recorded): Tracking.update's branches as they stand, c >= delay
// and c != delay + 1, or with QTOS_TRACK_CLEAN_DELAY c > delay.
__device__ inline bool track_recorded(long long c, int delay, bool clean) {
  return clean ? c > delay : (c >= delay && c != (long long)delay + 1);
}

template <int TILE>
__global__ __launch_bounds__(TILE) void k_track(const SamplePlan *Sd, TrackArgs A, const double *nodes, const double *t0,
                                                const int *first_row, const int *n_rows, const long long *cursor, const double *meas,
                                                const double *goal_x, long long *count, double *total, double *out, int *status_out,
                                                int B) {
  __shared__ double track_tile[TILE * TRACK_COLS];
  constexpr int FEET_LANE = TILE > 64 ? 64 : 0;                                    // the feet chain's owner: a lane of another wave
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long rows_b = G.rows_b, n = G.n;
  if (n == 0) return;                                                              // (uniform: a window without rows keeps its accumulators)
  const bool quat = (A.flags & 1) != 0, clean = (A.flags & 2) != 0;
  const int mcols = quat ? 19 : 18;
  const long long calls = count[2 * b];                                            // (every lane, in front of the first barrier)
  long long rec = count[2 * b + 1];
  double run = total[2 * b + (threadIdx.x == FEET_LANE && FEET_LANE ? 1 : 0)];     // the chain this lane owns, if it owns one
  double run_feet = total[2 * b + 1];                                              // (one wave: lane 0 owns both)
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  const double *meas_b = meas + (size_t)b * (size_t)rows_b * mcols;
  double *out_b = out + (size_t)b * (size_t)rows_b * TRACK_COLS;
  for (long long j0 = 0; j0 < n; j0 += TILE) {                                     // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, TILE);
    const long long base = G.row(j0);
    if ((int)threadIdx.x < m) {                                                    // (A) a lane takes a row
      double row[25];
      sample_row_state_at(S, x, t0b, G.plan_row(j0, threadIdx.x), A.hz, row);
      const long long o = G.tile_row(base, threadIdx.x);
      const double *mr = meas_b + (size_t)o * mcols;
      double *dst = track_tile + threadIdx.x * TRACK_COLS;
      double R[9];
      int st = track_pose(mr, quat, R, dst + 4);
      dst[0] = row[0];
      dst[1] = mr[0]; dst[2] = mr[1]; dst[3] = mr[2];
      dst[19] = track_norm(row + 1, mr);
      const double *q = mr + (quat ? 7 : 6);
      track_leg<0>(A, row, mr, R, q, dst);
      track_leg<1>(A, row, mr, R, q, dst);
      track_leg<2>(A, row, mr, R, q, dst);
      track_leg<3>(A, row, mr, R, q, dst);
      if (track_recorded(calls + j0 + threadIdx.x + 1, A.delay, clean)) st |= 1;
      if (goal_x && mr[0] >= goal_x[b]) st |= 2;
      status_out[(size_t)b * (size_t)rows_b + o] = st;
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                        // (B) the chains, in program order
      for (int i = 0; i < m; ++i) {
        double *r = track_tile + i * TRACK_COLS;
        if (track_recorded(calls + j0 + i + 1, A.delay, clean)) { run += r[19]; ++rec; }
        r[24] = run;
      }
    }
    if (threadIdx.x == FEET_LANE) {
      double f = FEET_LANE ? run : run_feet;
      for (int i = 0; i < m; ++i) {
        double *r = track_tile + i * TRACK_COLS;
        if (track_recorded(calls + j0 + i + 1, A.delay, clean)) { f += r[20]; f += r[21]; f += r[22]; f += r[23]; }
        r[25] = f;
      }
      if (FEET_LANE) run = f; else run_feet = f;
    }
    __syncthreads();
    segment_tile_out<TRACK_COLS>(G, base, m, track_tile, out_b, TILE);             // (C) the tile goes out flat
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    count[2 * b] = calls + n;
    count[2 * b + 1] = rec;
    total[2 * b] = run;
  }
  if (threadIdx.x == FEET_LANE) total[2 * b + 1] = FEET_LANE ? run : run_feet;
}

// Feedback hand-over (qtos_start_feedback*): the start vector k_handover wrote is corrected by the tracking error of the plan
// handed over from, so that the next plan starts where the robot is.  The statement of the rule is feedback.py.  One lane per
// window, as k_path_goal: the work of a window is one plan row (k_sample's evaluator), four legs (track_leg, k_track's own
// lines: the measured pose is k_track's columns 1 .. 18 to the bit) and four terrain look-ups (terrain_at, the solver's), a few
// hundred operations behind a launch; a wider layout was not measured.  Every function switches contraction off: one rounded
// operation per operation of the rule, in its order (the bilinear terrain_at keeps the solver's own build).  A window that
// falls back or has no measurement stores nothing to its start.  No LDS, no atomics, no scratch: the arrays of the arguments
// and the local vectors are indexed with constants only (templates over the leg, unrolled loops), the tables come through
// pointers.  No handle state is read or written but the sampling tables, the heightfields and their geometry.
struct FeedbackTerrain {   // what terrain_at reads of DevPlan
  const double *height;
  double hcell, hx0, hy0;
  int n_maps, hnx, hny, terrain_mode;
};
struct FeedbackArgs {   // QtosFeedback as the kernel reads it (window_api.hpp feedback_args)
  TrackArgs K;          // the leg chain, hz, the addressing and bit 0 of the flags (the quaternion), as k_track reads them
  FeedbackTerrain T;
  double gain_pos, gain_ang, gain_foot, max_pos, max_ang, max_foot;
  double nominal[NEE][3], max_deviation[3], rom_tol, snap_tol;
  int lat;              // round(latency * hz)
  int snap, zero_filter;
};

__device__ inline double feedback_clip(double e, double c, int &st) {   // a NaN stays a NaN
  if (e < -c) { st |= 2; return -c; }
  if (e > c) { st |= 2; return c; }
  return e;
}

// Foot E of the corrected start c (24 doubles): x and y by the gain, z by the gain or, with the snap, the terrain under the
// corrected x, y (status bit 6 + E where that moves z by more than snap_tol), then the range-of-motion test of the foot against
// the corrected base: d = R^T (foot - com) - nominal[E], false where a |d_i| is not within max_deviation[i] + rom_tol.
template <int E>
__device__ inline bool feedback_foot(const FeedbackArgs &A, int map, const double *s, const double *e, const double R[9], double *c,
                                     int &st) {
#pragma clang fp contract(off)
  constexpr int o = 6 + 3 * E;
  if (A.gain_foot != 0) {
    c[o] = s[o] + A.gain_foot * e[o];
    c[o + 1] = s[o + 1] + A.gain_foot * e[o + 1];
    c[o + 2] = s[o + 2] + A.gain_foot * e[o + 2];
  } else {
    c[o] = s[o]; c[o + 1] = s[o + 1]; c[o + 2] = s[o + 2];
  }
  if (A.snap) {
    const double z = terrain_at(A.T, map, c[o], c[o + 1]).h;
    if (fabs(z - c[o + 2]) > A.snap_tol) st |= 64 << E;
    c[o + 2] = z;
  }
  const double v0 = c[o] - c[0], v1 = c[o + 1] - c[1], v2 = c[o + 2] - c[2];
  const double d0 = ((R[0] * v0 + R[3] * v1) + R[6] * v2) - A.nominal[E][0];
  const double d1 = ((R[1] * v0 + R[4] * v1) + R[7] * v2) - A.nominal[E][1];
  const double d2 = ((R[2] * v0 + R[5] * v1) + R[8] * v2) - A.nominal[E][2];
  return fabs(d0) <= A.max_deviation[0] + A.rom_tol && fabs(d1) <= A.max_deviation[1] + A.rom_tol &&
         fabs(d2) <= A.max_deviation[2] + A.rom_tol;
}

__global__ __launch_bounds__(64) void k_start_feedback(const SamplePlan *Sd, FeedbackArgs A, const double *nodes, const double *t0,
                                                       const int *row_in, const long long *cursor, const double *meas,
                                                       const int *map_id, double *start, const double *goal_step, double *goal,
                                                       double *err_out, int *status, int B) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  // The window's places in the outputs, as lane values from the start: with the uniform pointers kept to the end, and with the
  // plan row evaluated in front of the legs (the sampling tables and the leg data live together), the scalar registers run out
  // and the kernel gets a scratch frame.
  double *sb = start + (size_t)b * QTOS_START_DOUBLES, *eo = err_out ? err_out + (size_t)b * 18 : nullptr;
  double *gb = goal_step ? goal + (size_t)b * 3 : nullptr;
  const double *gs = goal_step ? goal_step + (size_t)b * 3 : nullptr;
  int *stb = status + b;
  const int map = map_id ? map_id[b] : 0;
  const long long r = row_in[b];
  const RowSegment G = RowSegment::of(A.K.capacity, A.K.n_rows, A.K.first_row, nullptr, nullptr, cursor, b);
  long long k = r - A.lat;                                                            // the measured plan row
  if (k > G.first + r - 1) k = G.first + r - 1;
  if (k < G.first) k = G.first;
  const long long j = k - G.first;                                                    // its place in the segment
  if (r <= 0 || j >= G.rows_b) { *stb = 32; return; }                            // no measurement: nothing else is touched
  const bool quat = (A.K.flags & 1) != 0;
  const double *mr = meas + ((size_t)b * (size_t)G.rows_b + (size_t)G.row(j)) * (quat ? 19 : 18);
  double row[25] = {0}, dst[TRACK_COLS], R[9];   // (track_leg's error column against `row` is not used here: the row comes behind the legs)
  int st = track_pose(mr, quat, R, dst + 4);                                          // (bit 2: the pitch clip acted)
  dst[1] = mr[0]; dst[2] = mr[1]; dst[3] = mr[2];
  const double *q = mr + (quat ? 7 : 6);
  track_leg<0>(A.K, row, mr, R, q, dst);
  track_leg<1>(A.K, row, mr, R, q, dst);
  track_leg<2>(A.K, row, mr, R, q, dst);
  track_leg<3>(A.K, row, mr, R, q, dst);
  sample_row_state_at(S, nodes + (size_t)b * S.n_vars, t0[b], G.plan_row(j, 0), A.K.hz, row);
  double e[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) e[i] = dst[1 + i] - row[1 + i];
  e[5] = remainder(e[5], 6.283185307179586);
#pragma unroll
  for (int i = 0; i < 18; ++i) e[i] = feedback_clip(e[i], i < 3 ? A.max_pos : (i < 6 ? A.max_ang : A.max_foot), st);
  if (eo) {
#pragma unroll
    for (int i = 0; i < 18; ++i) eo[i] = e[i];
  }
  double s[QTOS_START_DOUBLES], c[QTOS_START_DOUBLES];
#pragma unroll
  for (int i = 0; i < QTOS_START_DOUBLES; ++i) { s[i] = sb[i]; c[i] = s[i]; }
  if (A.gain_pos != 0) {
#pragma unroll
    for (int i = 0; i < 3; ++i) c[i] = s[i] + A.gain_pos * e[i];
  }
  if (A.gain_ang != 0) {
#pragma unroll
    for (int i = 3; i < 6; ++i) c[i] = s[i] + A.gain_ang * e[i];
  }
  double Rc[9], unused[3];
  track_pose(c, false, Rc, unused);                                                   // R of the corrected Euler angles
  bool ok = feedback_foot<0>(A, map, s, e, Rc, c, st);
  ok = feedback_foot<1>(A, map, s, e, Rc, c, st) && ok;
  ok = feedback_foot<2>(A, map, s, e, Rc, c, st) && ok;
  ok = feedback_foot<3>(A, map, s, e, Rc, c, st) && ok;
  // (the fallback's goal comes from two loads of its own: with s[0] here the two branches end in the same load, the compiler
  // merges them into one load through a choice of two addresses, and s and c stay in scratch for it)
  double gx = sb[0], gy = sb[1];
  if (A.gain_pos == 0 && A.gain_ang == 0 && A.gain_foot == 0) {
    st &= 6;                                                                          // (uniform) nothing to add: the start stays, to the bit
  } else if (!ok) {
    st |= 8;                                                                          // fallback: the start stays as it is
  } else {
    st |= 1;
#pragma unroll
    for (int i = 0; i < QTOS_START_DOUBLES; ++i) {
      if (A.zero_filter && fabs(c[i]) < 1e-4) c[i] = 0.0;                             // QTOS/utils.py zero_filter
      if (i < 18 || A.zero_filter) sb[i] = c[i];
    }
    gx = c[0]; gy = c[1];
  }
  if (gs) {
    gb[0] = gx + gs[0];
    gb[1] = gy + gs[1];
  }
  *stb = st;
}

// Plan check (qtos_plan_check*): what a plan violates between its knots.  The solver holds the rows of its NLP at their own
// times only; this kernel evaluates the same rows -- Newton-Euler, range of motion, terrain, friction and unilateral force --
// at every sampled row, 27 columns per row, and reduces them to five families per window (max, the lowest row that attains
// it, the rows over a tolerance).  The statement of the rule is plan_check.py.  One workgroup per window walks its rows tile
// by tile, as k_track does: (A) a lane takes a row and puts its 27 values into the row's place of an LDS tile, keeping the
// five family violations in registers; (B) fifteen workgroup reductions (wg_reduce: max, then the lowest lane that attains
// it, then the count) whose results every lane merges into the running records it carries from tile to tile -- the results
// are uniform, so the records are scalars; (C) the tile goes out flat, consecutive lanes on consecutive doubles.  No atomics:
// max and count do not depend on the order and the row is the lowest one, so the summary is a function of the table alone
// and equals plan_check.summarise of it to the bit.  The arrays of the arguments are read with constant indices only
// (check_foot is a template over the foot), the tables come through a pointer (see k_handover).
constexpr int CHECK_COLS = 27, CHECK_TILE = 256, CHECK_FAMILIES = 5;
struct CheckRecord {   // one family of one window in d_summary
  double max;
  long long row, count;
};
struct CheckArgs {     // QtosPlanCheck as the kernel reads it, with the model's constants (window_api.hpp plan_check_args)
  double hz, mass, gravity, Ib[9], mu, f_max;
  double rom_lo[NEE][3], rom_hi[NEE][3];   // nominal_stance -+ max_dev, as the NLP's bounds are formed
  double tol[CHECK_FAMILIES];
  FeedbackTerrain T;
  const int *stance[NEE];                  // per foot and polynomial of its motion spline: 1 stance, 0 swing
  int first_row, n_rows, accumulate;
};

// The polynomial of time t: sample_spline's search, for the stance flag of a foot's motion spline.
__device__ inline int sample_segment(const SampleSpline &S, double t) {
  int lo = 0, hi = S.n_polys - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (S.tend[mid] >= t - 1e-10) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// The second derivative of a spline at time t: sample_spline's polynomial and local time with the weights of the second
// derivative.  A function of its own: sample_spline keeps the code k_sample, k_stitch and k_handover are held to bit for bit.
__device__ inline void sample_spline_acc(const SampleSpline &S, const double *x, double t, double out[3]) {
  const int k = sample_segment(S, t);
  const double T = S.dur[k];
  const double tau = t - (S.tend[k] - T);
  const double T2 = T * T, T3 = T2 * T;
  const double w[4] = {-6 / T2 + 12 * tau / T3, -4 / T + 6 * tau / T2, 6 / T2 - 12 * tau / T3, -2 / T + 6 * tau / T2};
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    double acc = 0;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int v = S.idx[(k + (a >> 1)) * 6 + (a & 1) * 3 + d];
      if (v >= 0) acc += w[a] * x[v];
    }
    out[d] = acc;
  }
}

__device__ inline double check_finite_or_inf(double v) { return isfinite(v) ? v : INFINITY; }

// Foot E of a check row: takes its force and lever arm off the dynamics rows ga, gl, writes the range-of-motion excess, the
// clearance and the force excess to dst (the row's place in the tile) and raises the three families' violations.
template <int E>
__device__ inline void check_foot(const SamplePlan &S, const CheckArgs &A, const double *x, double t, int map, const double r[3],
                                  const double R[9], double ga[3], double gl[3], double *dst, double &v_rom, double &v_terr,
                                  double &v_force) {
  double pe[3], f[3];
  sample_spline(S.eem[E], x, t, 0, pe);
  sample_spline(S.eef[E], x, t, 0, f);
  const bool stance = A.stance[E][sample_segment(S.eem[E], t)] != 0;
  const double d[3] = {r[0] - pe[0], r[1] - pe[1], r[2] - pe[2]};
  ga[0] -= f[1] * d[2] - f[2] * d[1];
  ga[1] -= f[2] * d[0] - f[0] * d[2];
  ga[2] -= f[0] * d[1] - f[1] * d[0];
  gl[0] -= f[0]; gl[1] -= f[1]; gl[2] -= f[2];
  // range of motion: g = R^T (p - r) against its box
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double g = -(R[i] * d[0] + R[3 + i] * d[1] + R[6 + i] * d[2]);
    const double ex = fmax(A.rom_lo[E][i] - g, g - A.rom_hi[E][i]);
    dst[7 + 3 * E + i] = ex;
    v_rom = fmax(v_rom, isfinite(ex) ? fmax(ex, 0.0) : INFINITY);
  }
  // terrain under the foot (a foot at a non-finite place has no terrain: the look-up would clamp it to a cell)
  Terr tr = terrain_at(A.T, map, pe[0], pe[1]);
  if (!(isfinite(pe[0]) && isfinite(pe[1]))) { tr.h = NAN; tr.hx = NAN; tr.hy = NAN; }
  const double c = pe[2] - tr.h;
  dst[19 + E] = c;
  v_terr = fmax(v_terr, isfinite(c) ? (stance ? fabs(c) : fmax(-c, 0.0)) : INFINITY);
  // force: the five rows of the NLP in a stance, max |f_i| in a swing
  double ex;
  if (stance) {
    double b[3][3], bx[3], by[3];
#pragma unroll
    for (int w = 0; w < 3; ++w) terrain_basis(tr, w, b[w], bx, by);
    // (the rows as eval_force forms them: the combined vector first, then its product with f)
    double g[5];
    g[0] = f[0] * b[0][0] + f[1] * b[0][1] + f[2] * b[0][2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const double s = (q & 1) ? A.mu : -A.mu;
      g[1 + q] = f[0] * (s * b[0][0] + b[1 + (q >> 1)][0]) + f[1] * (s * b[0][1] + b[1 + (q >> 1)][1]) +
                 f[2] * (s * b[0][2] + b[1 + (q >> 1)][2]);
    }
    ex = fmax(fmax(fmax(-g[0], g[0] - A.f_max), fmax(g[1], -g[2])), fmax(g[3], -g[4]));
    if (!(isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(g[3]) && isfinite(g[4]))) ex = NAN;
  } else {
    ex = fmax(fmax(fabs(f[0]), fabs(f[1])), fabs(f[2]));
    if (f[0] != f[0] || f[1] != f[1] || f[2] != f[2]) ex = NAN;
  }
  dst[23 + E] = ex;
  v_force = fmax(v_force, isfinite(ex) ? fmax(ex, 0.0) : INFINITY);
}

__global__ __launch_bounds__(CHECK_TILE) void k_plan_check(const SamplePlan *Sd, CheckArgs A, const double *nodes, const double *t0,
                                                           const int *map_id, const int *first_row, const int *n_rows,
                                                           const long long *cursor, double *rows_out, CheckRecord *summary, int B) {
  __shared__ double check_tile[CHECK_TILE * CHECK_COLS];
  __shared__ double check_red[CHECK_TILE];
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  // A table only, so RowSegment's count and first-row clamps and its plan row are spelled here: through RowSegment the same
  // lines compiled to 10 more spilled scalar registers, and the launch with per-window arrays measured up to 0.8 % slower
  // ("Row segments").
  long long n = n_rows ? n_rows[b] : A.n_rows;
  n = n < 0 ? 0 : (n > A.n_rows ? A.n_rows : n);
  long long first = first_row ? first_row[b] : A.first_row;
  first = first < 0 ? 0 : first;
  const long long row0 = cursor ? cursor[b] : first;                               // what the summary counts its rows from
  const int map = map_id ? map_id[b] : 0;
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)A.n_rows * CHECK_COLS : nullptr;
  double run_max[CHECK_FAMILIES];
  long long run_row[CHECK_FAMILIES], run_cnt[CHECK_FAMILIES];
#pragma unroll
  for (int f = 0; f < CHECK_FAMILIES; ++f) { run_max[f] = -INFINITY; run_row[f] = -1; run_cnt[f] = 0; }
  for (long long j0 = 0; j0 < n; j0 += CHECK_TILE) {                               // (n is uniform over the workgroup: so are the barriers)
    const int m = n - j0 < CHECK_TILE ? (int)(n - j0) : CHECK_TILE;
    double v[CHECK_FAMILIES];
#pragma unroll
    for (int f = 0; f < CHECK_FAMILIES; ++f) v[f] = -INFINITY;                     // a lane without a row: below every violation
    if ((int)threadIdx.x < m) {                                                    // (A) a lane takes a row
      const long long kk = first + j0 + threadIdx.x;
      const int k = kk > INT_MAX ? INT_MAX : (int)kk;
      double t = k / A.hz;
      if (t > S.T) t = S.T;
      double *dst = check_tile + threadIdx.x * CHECK_COLS;
      dst[0] = t0b + k / A.hz;                                                     // sample_row_state_at's time stamp
      double r[3], a[3], th[3], thd[3], thdd[3], ga[3], gl[3], R[9];
      sample_spline(S.lin, x, t, 0, r);
      sample_spline_acc(S.lin, x, t, a);
      sample_spline(S.ang, x, t, 0, th);
      sample_spline(S.ang, x, t, 1, thd);
      sample_spline_acc(S.ang, x, t, thdd);
      const Trig tg = trig_of(th);
      dyn_angular<double>(A.Ib, th, thd, thdd, tg, ga);
      rotation<double>(th, tg, R);
      gl[0] = A.mass * a[0]; gl[1] = A.mass * a[1]; gl[2] = A.mass * a[2] + A.mass * A.gravity;
      double v_rom = 0, v_terr = 0, v_force = 0;
      check_foot<0>(S, A, x, t, map, r, R, ga, gl, dst, v_rom, v_terr, v_force);
      check_foot<1>(S, A, x, t, map, r, R, ga, gl, dst, v_rom, v_terr, v_force);
      check_foot<2>(S, A, x, t, map, r, R, ga, gl, dst, v_rom, v_terr, v_force);
      check_foot<3>(S, A, x, t, map, r, R, ga, gl, dst, v_rom, v_terr, v_force);
      dst[1] = ga[0]; dst[2] = ga[1]; dst[3] = ga[2];
      dst[4] = gl[0]; dst[5] = gl[1]; dst[6] = gl[2];
      v[0] = fmax(fmax(check_finite_or_inf(fabs(ga[0])), check_finite_or_inf(fabs(ga[1]))), check_finite_or_inf(fabs(ga[2])));
      v[1] = fmax(fmax(check_finite_or_inf(fabs(gl[0])), check_finite_or_inf(fabs(gl[1]))), check_finite_or_inf(fabs(gl[2])));
      v[2] = v_rom; v[3] = v_terr; v[4] = v_force;
    }
    if (summary) {                                                                 // (B) the tile's families into the running records
#pragma unroll
      for (int f = 0; f < CHECK_FAMILIES; ++f) {
        const double mx = wg_reduce<1, CHECK_TILE>(v[f], check_red);               // (m >= 1: a violation, >= 0, is among them)
        const double at = wg_reduce<2, CHECK_TILE>(v[f] == mx ? (double)threadIdx.x : (double)CHECK_TILE, check_red);
        const double over = wg_reduce<0, CHECK_TILE>(v[f] > A.tol[f] ? 1.0 : 0.0, check_red);
        if (mx > run_max[f]) { run_max[f] = mx; run_row[f] = row0 + j0 + (long long)at; }
        run_cnt[f] += (long long)over;
      }
    }
    __syncthreads();
    if (out_b) {                                                                   // (C) the tile goes out flat
      double *o = out_b + (size_t)j0 * CHECK_COLS;
      for (int e = threadIdx.x; e < m * CHECK_COLS; e += CHECK_TILE) o[e] = check_tile[e];
    }
    __syncthreads();
  }
  if (summary && threadIdx.x == 0) {
    if (A.accumulate && n == 0) return;                                            // nothing to merge
#pragma unroll
    for (int f = 0; f < CHECK_FAMILIES; ++f) {
      CheckRecord rec = {run_max[f], run_row[f], run_cnt[f]};
      CheckRecord *dst = summary + (size_t)b * CHECK_FAMILIES + f;
      if (A.accumulate) {
        const CheckRecord old = *dst;
        if (!(rec.max > old.max)) { rec.max = old.max; rec.row = old.row; }
        rec.count += old.count;
      }
      *dst = rec;
    }
  }
}

// Rollout (qtos_rollout*): the windows' robots as simulated rigid bodies -- what scripts/run.py asks PyBullet for once per tick.
// The planner's own model, one rigid body under the plan's foot forces, a PD wrench towards the plan and an optional push, is
// integrated forward row by row; the states become the measured ring k_track and k_start_feedback read.  The statement of the
// rule is rollout.py, and every function below switches contraction off: one rounded operation per operation of the rule, in
// its order.  The state is a sequential chain by definition, so one workgroup owns one window and walks its tiles in order.
// Per tile: (A) a lane takes a row -- the plan row with k_sample's evaluator, then r_p, v_p, q_p, w_p, F, tau_p and the time
// stamp into the row's place of an LDS tile: all trigonometry of the plan is here, in parallel; (B) behind a barrier lane 0
// runs the chain over the tile's rows from the state it carries in registers: per row the state at the tick's start, |e|, the
// tilt, |F_fb| and the status bits go into the row's place, then the tick's substeps are taken (translation first, the rotation
// reads its e) -- only +, -, x, / and sqrt; (C) behind a barrier a lane turns its row's state into the 20 output columns (R from
// the quaternion, the Euler extraction of track_pose, R w_b) in the row's own place, and behind one more barrier the tile goes
// out flat, consecutive lanes on consecutive doubles: `rows` with its pitch of 20, `meas` with its 18 or 19 columns, the joint
// columns copied from the joint ring's row or left alone (RowSegment's addressing: table or ring, cursor and t0 only read).
// Carried state, count and word are read in front of the first barrier and written once by lane 0 behind the last tile; a
// window without rows keeps them (QTOS_ROLLOUT_PENDING in its word with them, until a call gives it rows).  The two chains are NOT split over two lanes or pipelined over tiles: the freeze (a fallen
// body stops both) couples them row by row, and the one-lane form was not measured against a split one.  No atomics, no
// scratch (the state and the body's constants are scalars and structs read with constant indices), no sincos.
struct RolloutArgs {   // QtosRollout as the kernel reads it (window_api.hpp rollout_args)
  double hz, h, mass, gravity, ff_scale, f_fb_max, t_fb_max, dev_max, tilt_max;
  double Ib[9], Ii[9], kp_lin[3], kd_lin[3], kp_ang[3], kd_ang[3];
  long long capacity, push_from, push_ticks;
  int first_row, n_rows, substeps, flags;
};
constexpr int ROLLOUT_COLS = 20;
constexpr int ROLLOUT_PITCH = 37;   // doubles per row of the tile: 20 inputs / outputs, 13 of the state, |e|, tilt, |F_fb|, status
constexpr int ROLLOUT_TILE = 256;   // rows per tile = lanes per workgroup: 256 x 37 x 8 = 75 776 bytes of LDS
constexpr int ROLLOUT_TICK = 64;    // one wave where no window has more rows (the tick): 18 944 bytes
struct RolloutState { double r0, r1, r2, v0, v1, v2, qx, qy, qz, qw, w0, w1, w2; };
struct RolloutBody { double m_s, I[9], J[9], F0, F1, F2, T0, T1, T2; };   // mass, inertia and its inverse scaled; the push

// A plan row c (37 columns) into the tile's 20 input columns (rollout.plan_inputs).
__device__ inline void rollout_inputs(const double *c, double ff, double *d) {
#pragma clang fp contract(off)
  d[0] = c[0]; d[1] = c[1]; d[2] = c[2]; d[3] = c[3]; d[4] = c[19]; d[5] = c[20]; d[6] = c[21];
  const double hr = c[4] * 0.5, hp = c[5] * 0.5, hy = c[6] * 0.5;
  const double sr = sin(hr), cr = cos(hr), sp = sin(hp), cp = cos(hp), sy = sin(hy), cy = cos(hy);
  d[7] = sr * cp * cy - cr * sp * sy; d[8] = cr * sp * cy + sr * cp * sy;
  d[9] = cr * cp * sy - sr * sp * cy; d[10] = cr * cp * cy + sr * sp * sy;
  const double sb = sin(c[5]), cb = cos(c[5]), sc = sin(c[6]), cc = cos(c[6]);
  d[11] = cb * cc * c[22] - sc * c[23]; d[12] = cb * sc * c[22] + cc * c[23]; d[13] = c[24] - sb * c[22];
  double F0 = 0, F1 = 0, F2 = 0, T0 = 0, T1 = 0, T2 = 0;
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    const double f0 = c[25 + 3 * e], f1 = c[26 + 3 * e], f2 = c[27 + 3 * e];
    const double d0 = c[7 + 3 * e] - c[1], d1 = c[8 + 3 * e] - c[2], d2 = c[9 + 3 * e] - c[3];
    const double x0 = d1 * f2 - d2 * f1, x1 = d2 * f0 - d0 * f2, x2 = d0 * f1 - d1 * f0;
    if (e == 0) { F0 = f0; F1 = f1; F2 = f2; T0 = x0; T1 = x1; T2 = x2; }
    else { F0 = F0 + f0; F1 = F1 + f1; F2 = F2 + f2; T0 = T0 + x0; T1 = T1 + x1; T2 = T2 + x2; }
  }
  d[14] = ff * F0; d[15] = ff * F1; d[16] = ff * F2; d[17] = ff * T0; d[18] = ff * T1; d[19] = ff * T2;
}

// sqrt((a a + b b) + c c)
__device__ inline double rollout_norm(double a, double b, double c) {
#pragma clang fp contract(off)
  return sqrt((a * a + b * b) + c * c);
}

// q_e = q_p (x) conj(q), negated if its w < 0 (rollout.attitude_error); p: the row's place in the tile.
__device__ inline void rollout_attitude(const double *p, const RolloutState &s, double &ex, double &ey, double &ez, double &ew) {
#pragma clang fp contract(off)
  const double px = p[7], py = p[8], pz = p[9], pw = p[10];
  const double x = -s.qx, y = -s.qy, z = -s.qz, w = s.qw;
  ex = ((pw * x + px * w) + py * z) - pz * y;
  ey = ((pw * y - px * z) + py * w) + pz * x;
  ez = ((pw * z + px * y) - py * x) + pz * w;
  ew = ((pw * w - px * x) - py * y) - pz * z;
  if (ew < 0) { ex = -ex; ey = -ey; ez = -ez; ew = -ew; }
}

__device__ inline double rollout_clip(double v, double lim, bool &acted) {   // a NaN stays a NaN
  if (lim > 0) {
    if (v < -lim) { acted = true; return -lim; }
    if (v > lim) { acted = true; return lim; }
  }
  return v;
}

// rollout_step's lines 1, 2 and 4 .. 7 and, below, 9 .. 11 as two functions of their own, for k_rollout_feet's step, which replaces
// the lines between them.  rollout_step itself keeps its one body: split into these calls k_rollout compiled to other code.
// Lines 1, 2 and 4 .. 7 of rollout.step under the row p: e, the clipped F_fb (b), R(q) and the clipped tau_fb (c).
__device__ inline void rollout_feedback(const RolloutArgs &A, const double *p, const RolloutState &s, double e[3], double b[3], double R[9],
                                        double c[3], bool &clipped) {
#pragma clang fp contract(off)
  e[0] = s.r0 - p[1]; e[1] = s.r1 - p[2]; e[2] = s.r2 - p[3];
  b[0] = rollout_clip(-(A.kp_lin[0] * e[0]) - A.kd_lin[0] * (s.v0 - p[4]), A.f_fb_max, clipped);
  b[1] = rollout_clip(-(A.kp_lin[1] * e[1]) - A.kd_lin[1] * (s.v1 - p[5]), A.f_fb_max, clipped);
  b[2] = rollout_clip(-(A.kp_lin[2] * e[2]) - A.kd_lin[2] * (s.v2 - p[6]), A.f_fb_max, clipped);
  const double x = s.qx, y = s.qy, z = s.qz, w = s.qw;
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
  double qx, qy, qz, qw;
  rollout_attitude(p, s, qx, qy, qz, qw);
  const double g0 = 2 * qx, g1 = 2 * qy, g2 = 2 * qz;
  const double u0 = (R[0] * s.w0 + R[1] * s.w1) + R[2] * s.w2, u1 = (R[3] * s.w0 + R[4] * s.w1) + R[5] * s.w2,
               u2 = (R[6] * s.w0 + R[7] * s.w1) + R[8] * s.w2;
  c[0] = rollout_clip(A.kp_ang[0] * g0 + A.kd_ang[0] * (p[11] - u0), A.t_fb_max, clipped);
  c[1] = rollout_clip(A.kp_ang[1] * g1 + A.kd_ang[1] * (p[12] - u1), A.t_fb_max, clipped);
  c[2] = rollout_clip(A.kp_ang[2] * g2 + A.kd_ang[2] * (p[13] - u2), A.t_fb_max, clipped);
}

// Lines 9 .. 11 of rollout.step: the state moved on by h under the acceleration a and the world torque t, R = R(q) of the old state.
__device__ inline void rollout_advance(const RolloutArgs &A, const RolloutBody &M, const double R[9], const double a[3], const double t[3],
                                       RolloutState &s) {
#pragma clang fp contract(off)
  const double h = A.h;
  const double x = s.qx, y = s.qy, z = s.qz, w = s.qw;
  s.v0 = s.v0 + h * a[0]; s.r0 = s.r0 + h * s.v0;
  s.v1 = s.v1 + h * a[1]; s.r1 = s.r1 + h * s.v1;
  s.v2 = s.v2 + h * a[2]; s.r2 = s.r2 + h * s.v2;
  const double tb0 = (R[0] * t[0] + R[3] * t[1]) + R[6] * t[2], tb1 = (R[1] * t[0] + R[4] * t[1]) + R[7] * t[2],
               tb2 = (R[2] * t[0] + R[5] * t[1]) + R[8] * t[2];
  const double i0 = (M.I[0] * s.w0 + M.I[1] * s.w1) + M.I[2] * s.w2, i1 = (M.I[3] * s.w0 + M.I[4] * s.w1) + M.I[5] * s.w2,
               i2 = (M.I[6] * s.w0 + M.I[7] * s.w1) + M.I[8] * s.w2;
  const double n0 = tb0 - (s.w1 * i2 - s.w2 * i1), n1 = tb1 - (s.w2 * i0 - s.w0 * i2), n2 = tb2 - (s.w0 * i1 - s.w1 * i0);
  const double w0 = s.w0 + h * ((M.J[0] * n0 + M.J[1] * n1) + M.J[2] * n2);
  const double w1 = s.w1 + h * ((M.J[3] * n0 + M.J[4] * n1) + M.J[5] * n2);
  const double w2 = s.w2 + h * ((M.J[6] * n0 + M.J[7] * n1) + M.J[8] * n2);
  const double hh = h * 0.5;
  const double d0 = (w * w0 + y * w2) - z * w1, d1 = (w * w1 - x * w2) + z * w0, d2 = (w * w2 + x * w1) - y * w0,
               d3 = (-(x * w0) - y * w1) - z * w2;
  const double m0 = x + hh * d0, m1 = y + hh * d1, m2 = z + hh * d2, m3 = w + hh * d3;
  const double nn = sqrt(((m0 * m0 + m1 * m1) + m2 * m2) + m3 * m3);
  s.qx = m0 / nn; s.qy = m1 / nn; s.qz = m2 / nn; s.qw = m3 / nn;
  s.w0 = w0; s.w1 = w1; s.w2 = w2;
}

// One step of length A.h under the row p (rollout.step, its lines 1 .. 11); returns |F_fb|.
__device__ inline double rollout_step(const RolloutArgs &A, const RolloutBody &M, const double *p, bool push, RolloutState &s,
                                      bool &clipped) {
#pragma clang fp contract(off)
  const double h = A.h;
  const double e0 = s.r0 - p[1], e1 = s.r1 - p[2], e2 = s.r2 - p[3];
  const double b0 = rollout_clip(-(A.kp_lin[0] * e0) - A.kd_lin[0] * (s.v0 - p[4]), A.f_fb_max, clipped);
  const double b1 = rollout_clip(-(A.kp_lin[1] * e1) - A.kd_lin[1] * (s.v1 - p[5]), A.f_fb_max, clipped);
  const double b2 = rollout_clip(-(A.kp_lin[2] * e2) - A.kd_lin[2] * (s.v2 - p[6]), A.f_fb_max, clipped);
  const double F0 = p[14], F1 = p[15], F2 = p[16];
  const double P0 = push ? M.F0 : 0.0, P1 = push ? M.F1 : 0.0, P2 = push ? M.F2 : 0.0;
  const double Q0 = push ? M.T0 : 0.0, Q1 = push ? M.T1 : 0.0, Q2 = push ? M.T2 : 0.0;
  const double a0 = ((F0 + b0) + P0) / M.m_s, a1 = ((F1 + b1) + P1) / M.m_s, a2 = ((F2 + b2) + P2) / M.m_s - A.gravity;
  const double x = s.qx, y = s.qy, z = s.qz, w = s.qw;
  const double R0 = 1 - 2 * (y * y + z * z), R1 = 2 * (x * y - z * w), R2 = 2 * (x * z + y * w);
  const double R3 = 2 * (x * y + z * w), R4 = 1 - 2 * (x * x + z * z), R5 = 2 * (y * z - x * w);
  const double R6 = 2 * (x * z - y * w), R7 = 2 * (y * z + x * w), R8 = 1 - 2 * (x * x + y * y);
  double qx, qy, qz, qw;
  rollout_attitude(p, s, qx, qy, qz, qw);
  const double g0 = 2 * qx, g1 = 2 * qy, g2 = 2 * qz;
  const double u0 = (R0 * s.w0 + R1 * s.w1) + R2 * s.w2, u1 = (R3 * s.w0 + R4 * s.w1) + R5 * s.w2,
               u2 = (R6 * s.w0 + R7 * s.w1) + R8 * s.w2;
  const double c0 = rollout_clip(A.kp_ang[0] * g0 + A.kd_ang[0] * (p[11] - u0), A.t_fb_max, clipped);
  const double c1 = rollout_clip(A.kp_ang[1] * g1 + A.kd_ang[1] * (p[12] - u1), A.t_fb_max, clipped);
  const double c2 = rollout_clip(A.kp_ang[2] * g2 + A.kd_ang[2] * (p[13] - u2), A.t_fb_max, clipped);
  const double x0 = e1 * F2 - e2 * F1, x1 = e2 * F0 - e0 * F2, x2 = e0 * F1 - e1 * F0;
  const double t0 = ((p[17] - x0) + c0) + Q0, t1 = ((p[18] - x1) + c1) + Q1, t2 = ((p[19] - x2) + c2) + Q2;
  s.v0 = s.v0 + h * a0; s.r0 = s.r0 + h * s.v0;
  s.v1 = s.v1 + h * a1; s.r1 = s.r1 + h * s.v1;
  s.v2 = s.v2 + h * a2; s.r2 = s.r2 + h * s.v2;
  const double tb0 = (R0 * t0 + R3 * t1) + R6 * t2, tb1 = (R1 * t0 + R4 * t1) + R7 * t2, tb2 = (R2 * t0 + R5 * t1) + R8 * t2;
  const double i0 = (M.I[0] * s.w0 + M.I[1] * s.w1) + M.I[2] * s.w2, i1 = (M.I[3] * s.w0 + M.I[4] * s.w1) + M.I[5] * s.w2,
               i2 = (M.I[6] * s.w0 + M.I[7] * s.w1) + M.I[8] * s.w2;
  const double n0 = tb0 - (s.w1 * i2 - s.w2 * i1), n1 = tb1 - (s.w2 * i0 - s.w0 * i2), n2 = tb2 - (s.w0 * i1 - s.w1 * i0);
  const double w0 = s.w0 + h * ((M.J[0] * n0 + M.J[1] * n1) + M.J[2] * n2);
  const double w1 = s.w1 + h * ((M.J[3] * n0 + M.J[4] * n1) + M.J[5] * n2);
  const double w2 = s.w2 + h * ((M.J[6] * n0 + M.J[7] * n1) + M.J[8] * n2);
  const double hh = h * 0.5;
  const double d0 = (w * w0 + y * w2) - z * w1, d1 = (w * w1 - x * w2) + z * w0, d2 = (w * w2 + x * w1) - y * w0,
               d3 = (-(x * w0) - y * w1) - z * w2;
  const double m0 = x + hh * d0, m1 = y + hh * d1, m2 = z + hh * d2, m3 = w + hh * d3;
  const double nn = sqrt(((m0 * m0 + m1 * m1) + m2 * m2) + m3 * m3);
  s.qx = m0 / nn; s.qy = m1 / nn; s.qz = m2 / nn; s.qw = m3 / nn;
  s.w0 = w0; s.w1 = w1; s.w2 = w2;
  return rollout_norm(b0, b1, b2);
}

// (C) of a row: the state in t[S .. S + 12] (k_rollout: 20 .. 32) becomes the output columns 1 .. 16 in t (17 .. 19 move up from
// S + 13 .. S + 15); returns the GIMBAL bit.  The Euler extraction is track_pose's, with comparisons for the clip so that a NaN
// stays one.
template <int S = 20>
__device__ inline int rollout_output(double *t) {
#pragma clang fp contract(off)
  const double r0 = t[S], r1 = t[S + 1], r2 = t[S + 2], v0 = t[S + 3], v1 = t[S + 4], v2 = t[S + 5];
  const double x = t[S + 6], y = t[S + 7], z = t[S + 8], w = t[S + 9], w0 = t[S + 10], w1 = t[S + 11], w2 = t[S + 12];
  const double R0 = 1 - 2 * (y * y + z * z), R1 = 2 * (x * y - z * w), R2 = 2 * (x * z + y * w);
  const double R3 = 2 * (x * y + z * w), R4 = 1 - 2 * (x * x + z * z), R5 = 2 * (y * z - x * w);
  const double R6 = 2 * (x * z - y * w), R7 = 2 * (y * z + x * w), R8 = 1 - 2 * (x * x + y * y);
  double sp = -R6;
  sp = sp < -1.0 ? -1.0 : (sp > 1.0 ? 1.0 : sp);
  t[1] = r0; t[2] = r1; t[3] = r2;
  t[4] = atan2(R7, R8); t[5] = asin(sp); t[6] = atan2(R3, R0);
  t[7] = v0; t[8] = v1; t[9] = v2;
  t[10] = (R0 * w0 + R1 * w1) + R2 * w2; t[11] = (R3 * w0 + R4 * w1) + R5 * w2; t[12] = (R6 * w0 + R7 * w1) + R8 * w2;
  t[13] = x; t[14] = y; t[15] = z; t[16] = w;
  t[17] = t[S + 13]; t[18] = t[S + 14]; t[19] = t[S + 15];
  return fabs(R6) >= 1 ? 4 : 0;
}

template <int TILE>
__global__ __launch_bounds__(TILE) void k_rollout(const SamplePlan *Sd, RolloutArgs A, const double *nodes, const double *t0,
                                                  const int *first_row, const int *n_rows, const long long *cursor,
                                                  const double *joint, const double *mass_scale, const double *push, double *state,
                                                  long long *count, int *word_io, double *meas, double *rows_out, int *status_out,
                                                  int B) {
  __shared__ double roll_tile[TILE * ROLLOUT_PITCH];
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const bool quat = (A.flags & 2) != 0;
  const int mcols = quat ? 19 : 18;
  RolloutState s;                                                                  // (every lane, in front of the first barrier)
  {
    const double *sb = state + (size_t)b * 13;
    s.r0 = sb[0]; s.r1 = sb[1]; s.r2 = sb[2]; s.v0 = sb[3]; s.v1 = sb[4]; s.v2 = sb[5];
    s.qx = sb[6]; s.qy = sb[7]; s.qz = sb[8]; s.qw = sb[9]; s.w0 = sb[10]; s.w1 = sb[11]; s.w2 = sb[12];
  }
  const long long calls = count[b];
  int word = word_io[b];
  RolloutBody M;
  {
#pragma clang fp contract(off)
    const double ms = mass_scale ? mass_scale[b] : 1.0;
    M.m_s = A.mass * ms;
#pragma unroll
    for (int i = 0; i < 9; ++i) { M.I[i] = ms * A.Ib[i]; M.J[i] = A.Ii[i] / ms; }
    const double *pb = push ? push + (size_t)b * 6 : nullptr;
    M.F0 = pb ? pb[0] : 0.0; M.F1 = pb ? pb[1] : 0.0; M.F2 = pb ? pb[2] : 0.0;
    M.T0 = pb ? pb[3] : 0.0; M.T1 = pb ? pb[4] : 0.0; M.T2 = pb ? pb[5] : 0.0;
  }
  // (the segment is formed here, behind the loads of the carried state: formed in front of them its scalars are live across
  // them, and the tick measured 0.5 - 2 % slower; DESIGN.md, "Row segments")
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long rows_b = G.rows_b, n = G.n;
  if (n == 0) return;                                                              // (uniform: a window without rows keeps its state)
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  double *meas_b = meas + (size_t)b * (size_t)rows_b * mcols;
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)rows_b * ROLLOUT_COLS : nullptr;
  const double *joint_b = joint ? joint + (size_t)b * (size_t)rows_b * QTOS_CSV_COLS : nullptr;
  for (long long j0 = 0; j0 < n; j0 += TILE) {                                     // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, TILE);
    const long long base = G.row(j0);
    if ((int)threadIdx.x < m) {                                                    // (A) a lane takes a row of the plan
      double row[QTOS_CSV_COLS];
      const double t = sample_row_state_at(S, x, t0b, G.plan_row(j0, threadIdx.x), A.hz, row);
      for (int e = 0; e < NEE; ++e) sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
      rollout_inputs(row, A.ff_scale, roll_tile + threadIdx.x * ROLLOUT_PITCH);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                        // (B) the chain, in program order
#pragma clang fp contract(off)
      // QTOS_ROLLOUT_INIT, or QTOS_ROLLOUT_PENDING in the window's own word (spent here, by the first call that gives the window
      // rows): r_p, v_p, q_p, R(q_p)^T w_p of the first row
      if (j0 == 0 && ((A.flags & 1) || (word & 32))) {
        word &= ~32;
        const double *p = roll_tile;
        s.r0 = p[1]; s.r1 = p[2]; s.r2 = p[3]; s.v0 = p[4]; s.v1 = p[5]; s.v2 = p[6];
        s.qx = p[7]; s.qy = p[8]; s.qz = p[9]; s.qw = p[10];
        const double qx = s.qx, qy = s.qy, qz = s.qz, qw = s.qw;
        const double R0 = 1 - 2 * (qy * qy + qz * qz), R1 = 2 * (qx * qy - qz * qw), R2 = 2 * (qx * qz + qy * qw);
        const double R3 = 2 * (qx * qy + qz * qw), R4 = 1 - 2 * (qx * qx + qz * qz), R5 = 2 * (qy * qz - qx * qw);
        const double R6 = 2 * (qx * qz - qy * qw), R7 = 2 * (qy * qz + qx * qw), R8 = 1 - 2 * (qx * qx + qy * qy);
        s.w0 = (R0 * p[11] + R3 * p[12]) + R6 * p[13];
        s.w1 = (R1 * p[11] + R4 * p[12]) + R7 * p[13];
        s.w2 = (R2 * p[11] + R5 * p[12]) + R8 * p[13];
      }
      for (int i = 0; i < m; ++i) {
        double *p = roll_tile + i * ROLLOUT_PITCH;
        double ex, ey, ez, ew;
        rollout_attitude(p, s, ex, ey, ez, ew);
        const double en = rollout_norm(s.r0 - p[1], s.r1 - p[2], s.r2 - p[3]);
        const double tilt = 2 * rollout_norm(ex, ey, ez);
        const bool finite = isfinite(s.r0) && isfinite(s.r1) && isfinite(s.r2) && isfinite(s.v0) && isfinite(s.v1) && isfinite(s.v2) &&
                            isfinite(s.qx) && isfinite(s.qy) && isfinite(s.qz) && isfinite(s.qw) && isfinite(s.w0) && isfinite(s.w1) &&
                            isfinite(s.w2);
        if (!finite) word |= 2;
        if ((A.dev_max > 0 && en > A.dev_max) || (A.tilt_max > 0 && tilt > A.tilt_max)) word |= 1;
        int st = word & 3;
        p[20] = s.r0; p[21] = s.r1; p[22] = s.r2; p[23] = s.v0; p[24] = s.v1; p[25] = s.v2;
        p[26] = s.qx; p[27] = s.qy; p[28] = s.qz; p[29] = s.qw; p[30] = s.w0; p[31] = s.w1; p[32] = s.w2;
        p[33] = en; p[34] = tilt;
        double fbn = 0;
        if (!st) {
          const long long c = calls + j0 + i;
          const bool acts = push != nullptr && c >= A.push_from && c - A.push_from < A.push_ticks;
          bool clipped = false;
          for (int u = 0; u < A.substeps; ++u) {
            const double f = rollout_step(A, M, p, acts, s, clipped);
            if (u == 0) fbn = f;
          }
          st = (clipped ? 8 : 0) | (acts ? 16 : 0);
        }
        p[35] = fbn; p[36] = (double)st;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < m) {                                                    // (C) a lane turns its row's state into the output columns
      double *p = roll_tile + threadIdx.x * ROLLOUT_PITCH;
      const int st = (int)p[36] | rollout_output(p);
      status_out[(size_t)b * (size_t)rows_b + G.tile_row(base, threadIdx.x)] = st;
    }
    __syncthreads();
    if (out_b) {                                                                   // the tile goes out flat: rows ...
      for (int e = threadIdx.x; e < m * ROLLOUT_COLS; e += TILE) {
        const int i = e / ROLLOUT_COLS, c = e - i * ROLLOUT_COLS;
        out_b[G.flat(base, ROLLOUT_COLS, e)] = roll_tile[i * ROLLOUT_PITCH + c];
      }
    }
    for (int e = threadIdx.x; e < m * mcols; e += TILE) {                          // ... and meas
      const int i = e / mcols, c = e - i * mcols;
      const double *p = roll_tile + i * ROLLOUT_PITCH;
      const long long o = G.flat(base, mcols, e);
      if (c < 3) meas_b[o] = p[1 + c];
      else if (c < mcols - 12) meas_b[o] = quat ? p[13 + (c - 3)] : p[4 + (c - 3)];
      else if (joint_b) meas_b[o] = joint_b[(size_t)G.tile_row(base, i) * QTOS_CSV_COLS + 1 + (c - (mcols - 12))];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *sb = state + (size_t)b * 13;
    sb[0] = s.r0; sb[1] = s.r1; sb[2] = s.r2; sb[3] = s.v0; sb[4] = s.v1; sb[5] = s.v2;
    sb[6] = s.qx; sb[7] = s.qy; sb[8] = s.qz; sb[9] = s.qw; sb[10] = s.w0; sb[11] = s.w1; sb[12] = s.w2;
    count[b] = calls + n;
    word_io[b] = word;
  }
}

// Force fit (qtos_force_fit*): the contact forces of every row made to supply the wrench the planned motion needs -- what
// k_plan_check measures as columns 1 .. 6, taken off the stance feet by one damped weighted least-squares solve per row ("force
// distribution").  The statement of the rule is force_fit.py, with the order of every operation of the solve.  One workgroup per
// window walks its rows tile by tile, as k_plan_check does: (A) a lane takes a row -- the plan's own dynamics rows with
// k_plan_check's pieces (sample_spline, sample_spline_acc, dyn_angular, rotation, terrain_at and the stance flag table), the ten
// sums of the 6 x 6 system over the stance feet, its unpivoted Cholesky in registers (21 entries, constant indices: the loops
// are unrolled, the feet come through a template as check_foot<E>), the corrections, the residual rows as rho - A df, the excess
// of the fitted forces and the feed-forward torques at the joint angles of the joint table's row -- and puts its 32 values into
// the row's place of an LDS tile (pitch 33 doubles: at 32 every lane of a wave would write the same bank); (B) twelve workgroup
// reductions (wg_reduce) into the four running records, uniform scalars; (C) the tile goes out flat, consecutive lanes on
// consecutive doubles, RowSegment's addressing: table or ring, cursor and t0 only read.  Without a joint table columns 20 .. 31
// are not written.  The status is one int per lane.  No atomics: the summary is a function of the rows (force_fit.summarise).
// fit_excess switches contraction off: it is the one piece numpy forms again from the table's columns, to the bit.
constexpr int FIT_COLS = 32, FIT_PITCH = 33, FIT_TILE = 256, FIT_FAMILIES = 4;
struct FitArgs {       // QtosForceFit as the kernel reads it, with the model's constants (window_api.hpp force_fit_args)
  double hz, mass, gravity, Ib[9], mu, f_max;
  double arm, damping, w_min, excess_tol, tol[FIT_FAMILIES];
  double lateral[NEE], l_upper, l_lower;
  FeedbackTerrain T;
  const int *stance[NEE];                  // per foot and polynomial of its motion spline: 1 stance, 0 swing
  long long capacity;
  int first_row, n_rows, accumulate;
};
struct FitFoot {       // one foot of a row, in registers: p = p_e - r, f the plan's force, df the correction
  double p[3], f[3], df[3], w, hx, hy;
  bool stance;
};
struct FitSums { double W, s0, s1, s2, q00, q01, q02, q11, q12, q22; };

// Foot E of a row: position, force and stance flag as check_foot takes them, its force and lever arm off the dynamics rows ga, gl
// (check_foot's lines), the terrain's slopes under it and max(normal . f, 0) of a stance foot (0 for a swing foot) into F.w.
template <int E>
__device__ inline void fit_foot_load(const SamplePlan &S, const FitArgs &A, const double *x, double t, int map, const double r[3],
                                     double ga[3], double gl[3], FitFoot &F) {
  double pe[3];
  sample_spline(S.eem[E], x, t, 0, pe);
  sample_spline(S.eef[E], x, t, 0, F.f);
  F.stance = A.stance[E][sample_segment(S.eem[E], t)] != 0;
  const double d[3] = {r[0] - pe[0], r[1] - pe[1], r[2] - pe[2]};
  ga[0] -= F.f[1] * d[2] - F.f[2] * d[1];
  ga[1] -= F.f[2] * d[0] - F.f[0] * d[2];
  ga[2] -= F.f[0] * d[1] - F.f[1] * d[0];
  gl[0] -= F.f[0]; gl[1] -= F.f[1]; gl[2] -= F.f[2];
  F.p[0] = pe[0] - r[0]; F.p[1] = pe[1] - r[1]; F.p[2] = pe[2] - r[2];
  Terr tr = terrain_at(A.T, map, pe[0], pe[1]);
  if (!(isfinite(pe[0]) && isfinite(pe[1]))) { tr.hx = NAN; tr.hy = NAN; }
  F.hx = tr.hx; F.hy = tr.hy;
  double b[3], bx[3], by[3];
  terrain_basis(tr, 0, b, bx, by);
  const double g = F.f[0] * b[0] + F.f[1] * b[1] + F.f[2] * b[2];
  F.w = F.stance && g > 0 ? g : 0.0;
  F.df[0] = 0; F.df[1] = 0; F.df[2] = 0;
}

// A stance foot's share of the ten sums: d = p / arm, W += w, s_i += w d_i, q_ij += (w d_i) d_j.
__device__ inline void fit_foot_sums(const FitFoot &F, double arm, FitSums &Q) {
  if (!F.stance) return;
  const double d0 = F.p[0] / arm, d1 = F.p[1] / arm, d2 = F.p[2] / arm;
  const double w0 = F.w * d0, w1 = F.w * d1, w2 = F.w * d2;
  Q.W += F.w; Q.s0 += w0; Q.s1 += w1; Q.s2 += w2;
  Q.q00 += w0 * d0; Q.q01 += w0 * d1; Q.q02 += w0 * d2; Q.q11 += w1 * d1; Q.q12 += w1 * d2; Q.q22 += w2 * d2;
}

__device__ constexpr int fit_ix(int i, int j) { return i * (i + 1) / 2 + j; }   // the lower triangle, row by row

// acc - a b of the solve below.  FitFused: under the compiler's default, which may fuse it (k_force_fit); FitExact: two rounded
// operations (k_rollout_feet, whose chain switches contraction off).
struct FitFused {
  static __device__ inline double nms(double acc, double a, double b) { return acc - a * b; }
};
struct FitExact {
  static __device__ inline double nms(double acc, double a, double b) {
#pragma clang fp contract(off)
    return acc - a * b;
  }
};

// y = M^-1 rhs by the unpivoted Cholesky of force_fit.py; M: the lower triangle, overwritten with L.
template <class Op = FitFused>
__device__ inline void fit_solve(double M[21], const double rhs[6], double y[6]) {
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double acc = M[fit_ix(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) acc = Op::nms(acc, M[fit_ix(j, k)], M[fit_ix(j, k)]);
    const double ljj = sqrt(acc);
    M[fit_ix(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double a = M[fit_ix(i, j)];
#pragma unroll
      for (int k = 0; k < j; ++k) a = Op::nms(a, M[fit_ix(i, k)], M[fit_ix(j, k)]);
      M[fit_ix(i, j)] = a / ljj;
    }
  }
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double acc = rhs[i];
#pragma unroll
    for (int k = 0; k < i; ++k) acc = Op::nms(acc, M[fit_ix(i, k)], z[k]);
    z[i] = acc / M[fit_ix(i, i)];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double acc = z[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) acc = Op::nms(acc, M[fit_ix(k, i)], y[k]);
    y[i] = acc / M[fit_ix(i, i)];
  }
}

// A stance foot's correction df = w (y_ang x d + y_lin), taken off the residual rows and added to the squared change.
__device__ inline void fit_foot_correct(FitFoot &F, double arm, const double y[6], double ra[3], double rl[3], double &sq) {
  if (!F.stance) return;
  const double d0 = F.p[0] / arm, d1 = F.p[1] / arm, d2 = F.p[2] / arm;
  F.df[0] = (y[1] * d2 - y[2] * d1 + y[3]) * F.w;
  F.df[1] = (y[2] * d0 - y[0] * d2 + y[4]) * F.w;
  F.df[2] = (y[0] * d1 - y[1] * d0 + y[5]) * F.w;
  ra[0] -= F.p[1] * F.df[2] - F.p[2] * F.df[1];
  ra[1] -= F.p[2] * F.df[0] - F.p[0] * F.df[2];
  ra[2] -= F.p[0] * F.df[1] - F.p[1] * F.df[0];
  rl[0] -= F.df[0]; rl[1] -= F.df[1]; rl[2] -= F.df[2];
  sq += F.df[0] * F.df[0] + F.df[1] * F.df[1] + F.df[2] * F.df[2];
}

// check_foot's excess of a stance foot on the force f: the NLP's five force rows with the terrain basis of the slopes hx, hy,
// plan_check.force_rows operation for operation (one rounded operation each); NaN where a row is not finite.
__device__ inline double fit_excess(const double f[3], double hx, double hy, double mu, double f_max) {
#pragma clang fp contract(off)
  const double nn = sqrt((hx * hx + hy * hy) + 1.0), n1 = sqrt((1.0 + 0.0) + hx * hx), n2 = sqrt((0.0 + 1.0) + hy * hy);
  const double bn[3] = {-hx / nn, -hy / nn, 1.0 / nn};
  const double b1[3] = {1.0 / n1, 0.0 / n1, hx / n1}, b2[3] = {0.0 / n2, 1.0 / n2, hy / n2};
  double g[5];
  g[0] = (f[0] * bn[0] + f[1] * bn[1]) + f[2] * bn[2];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const double s = (q & 1) ? mu : -mu;
    const double *bt = (q >> 1) ? b2 : b1;
    g[1 + q] = (f[0] * (s * bn[0] + bt[0]) + f[1] * (s * bn[1] + bt[1])) + f[2] * (s * bn[2] + bt[2]);
  }
  double ex = fmax(fmax(fmax(-g[0], g[0] - f_max), fmax(g[1], -g[2])), fmax(g[3], -g[4]));
  if (!(isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]) && isfinite(g[3]) && isfinite(g[4]))) ex = NAN;
  return ex;
}

// Foot E's fitted force into columns 1 + 3 E .. of dst, its excess into v_ex and the status, its feed-forward torques
// -J^T R^T f_fit at the joint angles q (joint_leg's lines; q null: the columns are left alone).
template <int E>
__device__ inline int fit_foot_out(const FitArgs &A, const FitFoot &F, bool bad, const double R[9], const double *q, double *dst,
                                   double &v_ex) {
  double f[3] = {F.f[0], F.f[1], F.f[2]};
  if (F.stance && !bad) { f[0] = F.f[0] + F.df[0]; f[1] = F.f[1] + F.df[1]; f[2] = F.f[2] + F.df[2]; }
  dst[1 + 3 * E] = f[0]; dst[2 + 3 * E] = f[1]; dst[3 + 3 * E] = f[2];
  int st = 0;
  if (F.stance) {
    const double ex = fit_excess(f, F.hx, F.hy, A.mu, A.f_max);
    if (ex > A.excess_tol) st = 8 << E;
    v_ex = fmax(v_ex, isfinite(ex) ? (ex > 0 ? ex : 0.0) : INFINITY);
  }
  if (q) {
    const double q1 = q[3 * E], q2 = q[3 * E + 1], q3 = q[3 * E + 2];
    const double d = A.lateral[E], lu = A.l_upper, ll = A.l_lower;
    const double s1 = sin(q1), c1 = cos(q1), s2 = sin(q2), c2 = cos(q2), s23 = sin(q2 + q3), c23 = cos(q2 + q3);
    const double x = -lu * s2 - ll * s23, hh = lu * c2 + ll * c23, ls = ll * s23, lc = ll * c23;
    const double fx = R[0] * f[0] + R[3] * f[1] + R[6] * f[2], fy = R[1] * f[0] + R[4] * f[1] + R[7] * f[2],
                 fz = R[2] * f[0] + R[5] * f[1] + R[8] * f[2];
    const double gy = c1 * fy + s1 * fz, gz = c1 * fz - s1 * fy;
    dst[20 + 3 * E] = -(hh * gy + d * gz); dst[21 + 3 * E] = hh * fx + x * gz; dst[22 + 3 * E] = lc * fx - ls * gz;
  }
  return st;
}

__global__ __launch_bounds__(FIT_TILE) void k_force_fit(const SamplePlan *Sd, FitArgs A, const double *nodes, const double *t0,
                                                        const int *map_id, const int *first_row, const int *n_rows,
                                                        const long long *cursor, const double *joint, const double *mass_scale,
                                                        double *rows_out, int *status_out, CheckRecord *summary, int B) {
  __shared__ double fit_tile[FIT_TILE * FIT_PITCH];
  __shared__ double fit_red[FIT_TILE];
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long n = G.n, rows_b = G.rows_b;
  const long long row0 = A.capacity > 0 ? cursor[b] : G.first;                       // what the summary counts its rows from
  const int map = map_id ? map_id[b] : 0;
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  const double ms = mass_scale ? mass_scale[b] : 1.0;
  const double m_s = A.mass * ms;
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)rows_b * FIT_COLS : nullptr;
  const double *joint_b = joint ? joint + (size_t)b * (size_t)rows_b * QTOS_CSV_COLS : nullptr;
  double run_max[FIT_FAMILIES];
  long long run_row[FIT_FAMILIES], run_cnt[FIT_FAMILIES];
#pragma unroll
  for (int f = 0; f < FIT_FAMILIES; ++f) { run_max[f] = -INFINITY; run_row[f] = -1; run_cnt[f] = 0; }
  for (long long j0 = 0; j0 < n; j0 += FIT_TILE) {                                   // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, FIT_TILE);
    const long long base = G.row(j0);
    double v[FIT_FAMILIES];
#pragma unroll
    for (int f = 0; f < FIT_FAMILIES; ++f) v[f] = -INFINITY;                         // a lane without a row: below every violation
    if ((int)threadIdx.x < m) {                                                      // (A) a lane takes a row
      const int k = G.plan_row(j0, threadIdx.x);
      double t = k / A.hz;
      if (t > S.T) t = S.T;
      double *dst = fit_tile + threadIdx.x * FIT_PITCH;
      dst[0] = t0b + k / A.hz;                                                       // sample_row_state_at's time stamp
      double r[3], a[3], th[3], thd[3], thdd[3], ga[3], gl[3], R[9], Ib[9];
      sample_spline(S.lin, x, t, 0, r);
      sample_spline_acc(S.lin, x, t, a);
      sample_spline(S.ang, x, t, 0, th);
      sample_spline(S.ang, x, t, 1, thd);
      sample_spline_acc(S.ang, x, t, thdd);
      const Trig tg = trig_of(th);
#pragma unroll
      for (int i = 0; i < 9; ++i) Ib[i] = ms * A.Ib[i];
      dyn_angular<double>(Ib, th, thd, thdd, tg, ga);
      rotation<double>(th, tg, R);
      gl[0] = m_s * a[0]; gl[1] = m_s * a[1]; gl[2] = m_s * a[2] + m_s * A.gravity;
      FitFoot F0, F1, F2, F3;
      fit_foot_load<0>(S, A, x, t, map, r, ga, gl, F0);
      fit_foot_load<1>(S, A, x, t, map, r, ga, gl, F1);
      fit_foot_load<2>(S, A, x, t, map, r, ga, gl, F2);
      fit_foot_load<3>(S, A, x, t, map, r, ga, gl, F3);
      // the weights: F.w holds max(g, 0) of a stance foot
      const int cnt = (int)F0.stance + (int)F1.stance + (int)F2.stance + (int)F3.stance;
      const double nn = (double)cnt, gsum = ((F0.w + F1.w) + F2.w) + F3.w;
      const bool loaded = gsum > 0;
      F0.w = loaded ? fmax(nn * F0.w / gsum, A.w_min) : 1.0;
      F1.w = loaded ? fmax(nn * F1.w / gsum, A.w_min) : 1.0;
      F2.w = loaded ? fmax(nn * F2.w / gsum, A.w_min) : 1.0;
      F3.w = loaded ? fmax(nn * F3.w / gsum, A.w_min) : 1.0;
      double y[6] = {0, 0, 0, 0, 0, 0}, sq = 0;
      if (cnt > 0) {
        FitSums Q = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        fit_foot_sums(F0, A.arm, Q);
        fit_foot_sums(F1, A.arm, Q);
        fit_foot_sums(F2, A.arm, Q);
        fit_foot_sums(F3, A.arm, Q);
        const double lam = A.damping * nn, wl = Q.W + lam;
        double M[21] = {(Q.q11 + Q.q22) + lam,
                        -Q.q01, (Q.q00 + Q.q22) + lam,
                        -Q.q02, -Q.q12, (Q.q00 + Q.q11) + lam,
                        0.0, Q.s2, -Q.s1, wl,
                        -Q.s2, 0.0, Q.s0, 0.0, wl,
                        Q.s1, -Q.s0, 0.0, 0.0, 0.0, wl};
        const double rhs[6] = {ga[0] / A.arm, ga[1] / A.arm, ga[2] / A.arm, gl[0], gl[1], gl[2]};
        fit_solve(M, rhs, y);
      }
      fit_foot_correct(F0, A.arm, y, ga, gl, sq);
      fit_foot_correct(F1, A.arm, y, ga, gl, sq);
      fit_foot_correct(F2, A.arm, y, ga, gl, sq);
      fit_foot_correct(F3, A.arm, y, ga, gl, sq);
      const double change = sqrt(sq);
      bool fin = isfinite(ga[0]) && isfinite(ga[1]) && isfinite(ga[2]) && isfinite(gl[0]) && isfinite(gl[1]) && isfinite(gl[2]) &&
                 isfinite(change);
      fin = fin && isfinite(F0.df[0]) && isfinite(F0.df[1]) && isfinite(F0.df[2]) && isfinite(F1.df[0]) && isfinite(F1.df[1]) &&
            isfinite(F1.df[2]) && isfinite(F2.df[0]) && isfinite(F2.df[1]) && isfinite(F2.df[2]) && isfinite(F3.df[0]) &&
            isfinite(F3.df[1]) && isfinite(F3.df[2]);
      const bool bad = !fin;
      dst[13] = bad ? NAN : ga[0]; dst[14] = bad ? NAN : ga[1]; dst[15] = bad ? NAN : ga[2];
      dst[16] = bad ? NAN : gl[0]; dst[17] = bad ? NAN : gl[1]; dst[18] = bad ? NAN : gl[2];
      dst[19] = bad ? NAN : change;
      const double *q = joint_b ? joint_b + (size_t)G.tile_row(base, threadIdx.x) * QTOS_CSV_COLS + 1 : nullptr;
      double v_ex = 0;
      int st = (cnt == 0 ? 1 : 0) | (cnt == 2 ? 2 : 0) | (bad ? 4 : 0);
      st |= fit_foot_out<0>(A, F0, bad, R, q, dst, v_ex);
      st |= fit_foot_out<1>(A, F1, bad, R, q, dst, v_ex);
      st |= fit_foot_out<2>(A, F2, bad, R, q, dst, v_ex);
      st |= fit_foot_out<3>(A, F3, bad, R, q, dst, v_ex);
      if (status_out) status_out[(size_t)b * (size_t)rows_b + G.tile_row(base, threadIdx.x)] = st;
      v[0] = bad ? INFINITY : fmax(fmax(fabs(ga[0]), fabs(ga[1])), fabs(ga[2]));
      v[1] = bad ? INFINITY : fmax(fmax(fabs(gl[0]), fabs(gl[1])), fabs(gl[2]));
      v[2] = bad ? INFINITY : change;
      v[3] = v_ex;
    }
    if (summary) {                                                                   // (B) the tile's families into the running records
#pragma unroll
      for (int f = 0; f < FIT_FAMILIES; ++f) {
        const double mx = wg_reduce<1, FIT_TILE>(v[f], fit_red);                     // (m >= 1: a violation, >= 0, is among them)
        const double at = wg_reduce<2, FIT_TILE>(v[f] == mx ? (double)threadIdx.x : (double)FIT_TILE, fit_red);
        const double over = wg_reduce<0, FIT_TILE>(v[f] > A.tol[f] ? 1.0 : 0.0, fit_red);
        if (mx > run_max[f]) { run_max[f] = mx; run_row[f] = row0 + j0 + (long long)at; }
        run_cnt[f] += (long long)over;
      }
    }
    __syncthreads();
    if (out_b) {                                                                     // (C) the tile goes out flat
      for (int e = threadIdx.x; e < m * FIT_COLS; e += FIT_TILE) {
        const int i = e / FIT_COLS, c = e - i * FIT_COLS;
        if (c < 20 || joint_b) out_b[G.flat(base, FIT_COLS, e)] = fit_tile[i * FIT_PITCH + c];
      }
    }
    __syncthreads();
  }
  if (summary && threadIdx.x == 0) {
    if (A.accumulate && n == 0) return;                                              // nothing to merge
#pragma unroll
    for (int f = 0; f < FIT_FAMILIES; ++f) {
      CheckRecord rec = {run_max[f], run_row[f], run_cnt[f]};
      CheckRecord *dst = summary + (size_t)b * FIT_FAMILIES + f;
      if (A.accumulate) {
        const CheckRecord old = *dst;
        if (!(rec.max > old.max)) { rec.max = old.max; rec.row = old.row; }
        rec.count += old.count;
      }
      *dst = rec;
    }
  }
}

// Force QP (qtos_force_qp*): the force fit inside the friction pyramid.  The statement of the rule is force_qp.py, with the order
// of every operation; this kernel runs that order with contraction off (qp_* below; the row's plan side is k_force_fit's device
// functions, one copy of each, with fit_solve<FitExact>).  A row whose fitted forces obey the six limit rows of every stance foot
// is the fit's row; any other is the central point of the barrier problem at mu_end, by a feasible-start primal-dual iteration
// of at most 25 steps, each with one unpivoted 12 x 12 Cholesky.  One workgroup of QP_TILE = 128 lanes per window, one lane per
// row, k_force_fit's three phases.  What a lane carries through the iteration -- x, s, z, the feet's bases, lever arms, forces
// and weights, about 200 doubles -- stays in registers (constant indices: the loops over feet and limit rows are unrolled); the
// 78 entries of K and the 12 of the solves' vector live in a per-lane LDS slab, entry k of lane l at k * QP_TILE + l: consecutive
// lanes on consecutive doubles, so a wave's access to one entry is conflict-free, and the factorisation's loops stay rolled with
// run-time indices, which registers cannot take.  Every loop has a fixed bound; a NaN fails every comparison and runs into the
// cap; nothing spins on memory.  The lanes of a wave whose rows took the fit path wait for those that did not.
constexpr int QP_COLS = 8, QP_PITCH = 9, QP_TILE = 128, QP_SLAB = 90, QP_MAX_ITER = 25;
constexpr double QP_CTOL = 1e-10, QP_RTOL = 1e-9;                                     // force_qp.CTOL, RTOL
struct QpArgs { double mu, f_max, mu_end, act_tol; int max_iter; };
struct QpFoot {        // one foot of a row as the iteration reads it
  double d[3], w, f[3], B[3][3];
  bool on;
};
__device__ constexpr int qp_ix(int i, int j) { return i * (i + 1) / 2 + j; }

__device__ inline double qp_dot(const double u[3], const double v[3]) {
#pragma clang fp contract(off)
  return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
}
__device__ inline void qp_basis(double hx, double hy, double B[3][3]) {
#pragma clang fp contract(off)
  const double v[3][3] = {{-hx, -hy, 1.0}, {1.0, 0.0, hx}, {0.0, 1.0, hy}};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double nn = sqrt((v[a][0] * v[a][0] + v[a][1] * v[a][1]) + v[a][2] * v[a][2]);
    B[a][0] = v[a][0] / nn; B[a][1] = v[a][1] / nn; B[a][2] = v[a][2] / nn;
  }
}
__device__ inline void qp_gmul(const double B[3][3], double mu, const double v[3], double out[6]) {
#pragma clang fp contract(off)
  const double a = qp_dot(B[0], v), b = qp_dot(B[1], v), c2 = qp_dot(B[2], v), ma = mu * a;
  out[0] = -a; out[1] = a; out[2] = b - ma; out[3] = -(b + ma); out[4] = c2 - ma; out[5] = -(c2 + ma);
}
__device__ inline void qp_gtmul(const double B[3][3], double mu, const double y[6], double out[3]) {
#pragma clang fp contract(off)
  const double al = (y[1] - y[0]) - mu * (((y[2] + y[3]) + y[4]) + y[5]), be = y[2] - y[3], ga = y[4] - y[5];
#pragma unroll
  for (int i = 0; i < 3; ++i) out[i] = (B[0][i] * al + B[1][i] * be) + B[2][i] * ga;
}
// grad_e = (c / w_e) x_e - ((r~_ang x d_e) + r~_lin), r~ = rho~ - sum_S (d_e x x_e, x_e); 0 for a swing foot.
__device__ inline void qp_grad(const QpFoot Ft[NEE], const double rho[6], double c, const double x[NEE][3], double g[NEE][3]) {
#pragma clang fp contract(off)
  double r[6] = {rho[0], rho[1], rho[2], rho[3], rho[4], rho[5]};
#pragma unroll
  for (int e = 0; e < NEE; ++e)
    if (Ft[e].on) {
      const double *d = Ft[e].d, *v = x[e];
      r[0] = r[0] - (d[1] * v[2] - d[2] * v[1]);
      r[1] = r[1] - (d[2] * v[0] - d[0] * v[2]);
      r[2] = r[2] - (d[0] * v[1] - d[1] * v[0]);
      r[3] = r[3] - v[0]; r[4] = r[4] - v[1]; r[5] = r[5] - v[2];
    }
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    g[e][0] = 0; g[e][1] = 0; g[e][2] = 0;
    if (Ft[e].on) {
      const double *d = Ft[e].d;
      const double cw = c / Ft[e].w;
      g[e][0] = cw * x[e][0] - ((r[1] * d[2] - r[2] * d[1]) + r[3]);
      g[e][1] = cw * x[e][1] - ((r[2] * d[0] - r[0] * d[2]) + r[4]);
      g[e][2] = cw * x[e][2] - ((r[0] * d[1] - r[1] * d[0]) + r[5]);
    }
  }
}
// K = H + G^T diag(z / s) G into the lane's slab (the lower triangle, row by row), then its unpivoted Cholesky in place.
template <int STRIDE = QP_TILE>
__device__ inline void qp_factor(const QpFoot Ft[NEE], double c, double mu, const double s[NEE][6], const double z[NEE][6], double *K) {
#pragma clang fp contract(off)
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    double blk[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (Ft[e].on) {
      double D[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) D[r] = z[e][r] / s[e][r];
      const double S = ((D[2] + D[3]) + D[4]) + D[5];
      const double cnn = (D[0] + D[1]) + (mu * mu) * S, cn1 = mu * (D[3] - D[2]), cn2 = mu * (D[5] - D[4]), c11 = D[2] + D[3], c22 = D[4] + D[5];
      const double(*B)[3] = Ft[e].B;
      double Tn[3], T1[3], T2[3];
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        Tn[j] = (cnn * B[0][j] + cn1 * B[1][j]) + cn2 * B[2][j];
        T1[j] = cn1 * B[0][j] + c11 * B[1][j];
        T2[j] = cn2 * B[0][j] + c22 * B[2][j];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j <= i; ++j) blk[i][j] = (B[0][i] * Tn[j] + B[1][i] * T1[j]) + B[2][i] * T2[j];
    }
#pragma unroll
    for (int e2 = 0; e2 <= e; ++e2) {
      const bool both = Ft[e].on && Ft[e2].on;
      const double dd = qp_dot(Ft[e].d, Ft[e2].d);
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (e == e2 && j > i) continue;
          double v = -(Ft[e2].d[i] * Ft[e].d[j]);
          if (i == j) {
            v = (dd + 1.0) - Ft[e2].d[i] * Ft[e].d[j];
            if (e == e2) v = v + c / Ft[e].w;
          }
          double k = both ? v : (e == e2 && i == j ? 1.0 : 0.0);
          if (e == e2 && Ft[e].on) k = k + blk[i][j];
          K[qp_ix(3 * e + i, 3 * e2 + j) * STRIDE] = k;
        }
    }
  }
  for (int j = 0; j < 12; ++j) {
    double acc = K[qp_ix(j, j) * STRIDE];
    for (int k = 0; k < j; ++k) {
      const double l = K[qp_ix(j, k) * STRIDE];
      acc = acc - l * l;
    }
    const double ljj = sqrt(acc);
    K[qp_ix(j, j) * STRIDE] = ljj;
    for (int i = j + 1; i < 12; ++i) {
      double a = K[qp_ix(i, j) * STRIDE];
      for (int k = 0; k < j; ++k) a = a - K[qp_ix(i, k) * STRIDE] * K[qp_ix(j, k) * STRIDE];
      K[qp_ix(i, j) * STRIDE] = a / ljj;
    }
  }
}
// v = K^-1 v with the factor in the slab: v is the slab's entries 78 .. 89, in place.
template <int STRIDE = QP_TILE>
__device__ inline void qp_backsolve(double *K, double v[NEE][3]) {
#pragma clang fp contract(off)
  double *V = K + 78 * STRIDE;
#pragma unroll
  for (int e = 0; e < NEE; ++e)
#pragma unroll
    for (int i = 0; i < 3; ++i) V[(3 * e + i) * STRIDE] = v[e][i];
  for (int i = 0; i < 12; ++i) {
    double acc = V[i * STRIDE];
    for (int k = 0; k < i; ++k) acc = acc - K[qp_ix(i, k) * STRIDE] * V[k * STRIDE];
    V[i * STRIDE] = acc / K[qp_ix(i, i) * STRIDE];
  }
  for (int i = 11; i >= 0; --i) {
    double acc = V[i * STRIDE];
    for (int k = i + 1; k < 12; ++k) acc = acc - K[qp_ix(k, i) * STRIDE] * V[k * STRIDE];
    V[i * STRIDE] = acc / K[qp_ix(i, i) * STRIDE];
  }
#pragma unroll
  for (int e = 0; e < NEE; ++e)
#pragma unroll
    for (int i = 0; i < 3; ++i) v[e][i] = V[(3 * e + i) * STRIDE];
}
// Foot e's six rows of a step dx: ds = -G dx, dz = t - (z / s) ds (t = -z for the predictor, rc / s for the combined step).
__device__ inline void qp_foot_step(const QpFoot &F, double mu, const double dx[3], const double s[6], const double z[6], const double t[6],
                                    double ds[6], double dz[6]) {
#pragma clang fp contract(off)
  double gd[6];
  qp_gmul(F.B, mu, dx, gd);
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    ds[r] = -gd[r];
    dz[r] = t[r] - (z[r] / s[r]) * ds[r];
  }
}
// The limited path of a row (force_qp.solve_rows): x, s, z of the last iterate, the residuals it stopped at; returns the steps.
// STRIDE: the distance between two entries of the lane's slab K (QP_TILE: k_force_qp's lanes side by side; 1: a slab of one lane's own).
template <int STRIDE = QP_TILE>
__device__ inline int qp_solve(const QpFoot Ft[NEE], const double rho[6], double c, double m, const QpArgs &Q, const double xfit[NEE][3],
                               double *K, double x[NEE][3], double s[NEE][6], double z[NEE][6], double &comp, double &rdn, bool &cap) {
#pragma clang fp contract(off)
  const double mu = Q.mu, mu_end = Q.mu_end, inf = INFINITY;
  const double gam_lo = fmin(1.0, Q.f_max / 4.0), gam_hi = Q.f_max / 2.0;
  {                                                                                   // the start
    double xi[NEE][3], si[NEE][6], ratio = inf;
#pragma unroll
    for (int e = 0; e < NEE; ++e) {
      xi[e][0] = 0; xi[e][1] = 0; xi[e][2] = 0;
      if (Ft[e].on) {
        const double gam = fmin(fmax(qp_dot(Ft[e].B[0], Ft[e].f), gam_lo), gam_hi);
        double tmp[3], dir[3], gv[6], gd[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          xi[e][i] = Ft[e].B[0][i] * gam - Ft[e].f[i];
          tmp[i] = Ft[e].f[i] + xi[e][i];
          dir[i] = xfit[e][i] - xi[e][i];
        }
        qp_gmul(Ft[e].B, mu, tmp, gv);
        qp_gmul(Ft[e].B, mu, dir, gd);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          si[e][r] = (r == 1 ? Q.f_max : 0.0) - gv[r];
          if (-gd[r] < 0) ratio = fmin(ratio, si[e][r] / gd[r]);
        }
      }
    }
    const double theta = fmin(1.0, 0.9 * ratio);
#pragma unroll
    for (int e = 0; e < NEE; ++e) {
#pragma unroll
      for (int r = 0; r < 6; ++r) { s[e][r] = 1.0; z[e][r] = 1.0; }
      x[e][0] = 0; x[e][1] = 0; x[e][2] = 0;
      if (Ft[e].on) {
        double tmp[3], gv[6];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          x[e][i] = xi[e][i] + theta * (xfit[e][i] - xi[e][i]);
          tmp[i] = Ft[e].f[i] + x[e][i];
        }
        qp_gmul(Ft[e].B, mu, tmp, gv);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          s[e][r] = (r == 1 ? Q.f_max : 0.0) - gv[r];
          z[e][r] = 1.0 / s[e][r];
        }
      }
    }
  }
  double qinf = 0;
  {
    const double x0[NEE][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    double q[NEE][3];
    qp_grad(Ft, rho, c, x0, q);
#pragma unroll
    for (int e = 0; e < NEE; ++e) qinf = fmax(qinf, fmax(fmax(fabs(q[e][0]), fabs(q[e][1])), fabs(q[e][2])));
  }
  const int max_iter = Q.max_iter < QP_MAX_ITER ? Q.max_iter : QP_MAX_ITER;
  int steps = 0;
  cap = false;
  for (int it = 0; it <= QP_MAX_ITER; ++it) {
    double grad[NEE][3], rd[NEE][3], acc = 0, comp_now = 0, rd_now = 0;
    qp_grad(Ft, rho, c, x, grad);
#pragma unroll
    for (int e = 0; e < NEE; ++e) {
      rd[e][0] = 0; rd[e][1] = 0; rd[e][2] = 0;
      if (Ft[e].on) {
        double gt[3];
        qp_gtmul(Ft[e].B, mu, z[e], gt);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          rd[e][i] = grad[e][i] + gt[i];
          rd_now = fmax(rd_now, fabs(rd[e][i]));
        }
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          const double sz = s[e][r] * z[e][r];
          acc = acc + sz;
          comp_now = fmax(comp_now, fabs(sz - mu_end));
        }
      }
    }
    comp_now = comp_now / mu_end;
    const double muk = acc / m;
    comp = comp_now; rdn = rd_now;
    if (comp_now <= QP_CTOL && rd_now <= QP_RTOL * (1.0 + qinf)) break;
    if (it >= max_iter) { cap = true; break; }
    qp_factor<STRIDE>(Ft, c, mu, s, z, K);
    double t[NEE][6], dx[NEE][3];
    double target = mu_end;
    const bool pred = muk > 10.0 * mu_end;
    if (pred) {                                                                       // the predictor and the corrector's target
#pragma unroll
      for (int e = 0; e < NEE; ++e)
#pragma unroll
        for (int i = 0; i < 3; ++i) dx[e][i] = -grad[e][i];
      qp_backsolve<STRIDE>(K, dx);
      double rs = inf, rz = inf;
#pragma unroll
      for (int e = 0; e < NEE; ++e)
        if (Ft[e].on) {
          double ta[6], ds[6], dz[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) ta[r] = -z[e][r];
          qp_foot_step(Ft[e], mu, dx[e], s[e], z[e], ta, ds, dz);
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            if (ds[r] < 0) rs = fmin(rs, s[e][r] / -ds[r]);
            if (dz[r] < 0) rz = fmin(rz, z[e][r] / -dz[r]);
            t[e][r] = ds[r] * dz[r];                                                  // (the corrector's term, kept for rc below)
          }
        }
      const double ala = fmin(1.0, fmin(rs, rz));
      double acc_a = 0;
#pragma unroll
      for (int e = 0; e < NEE; ++e)
        if (Ft[e].on) {
          double ta[6], ds[6], dz[6];
#pragma unroll
          for (int r = 0; r < 6; ++r) ta[r] = -z[e][r];
          qp_foot_step(Ft[e], mu, dx[e], s[e], z[e], ta, ds, dz);
#pragma unroll
          for (int r = 0; r < 6; ++r) acc_a = acc_a + (s[e][r] + ala * ds[r]) * (z[e][r] + ala * dz[r]);
        }
      const double ratio = (acc_a / m) / muk;
      target = fmax(((ratio * ratio) * ratio) * muk, mu_end);
    }
#pragma unroll
    for (int e = 0; e < NEE; ++e) {
      dx[e][0] = -0.0; dx[e][1] = -0.0; dx[e][2] = -0.0;
      if (Ft[e].on) {
        double gt[3];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          double rc = target - s[e][r] * z[e][r];
          if (pred) rc = rc - t[e][r];
          t[e][r] = rc / s[e][r];
        }
        qp_gtmul(Ft[e].B, mu, t[e], gt);
#pragma unroll
        for (int i = 0; i < 3; ++i) dx[e][i] = -(rd[e][i] + gt[i]);
      }
    }
    qp_backsolve<STRIDE>(K, dx);
    double rs = inf, rz = inf;
#pragma unroll
    for (int e = 0; e < NEE; ++e)
      if (Ft[e].on) {
        double ds[6], dz[6];
        qp_foot_step(Ft[e], mu, dx[e], s[e], z[e], t[e], ds, dz);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          if (ds[r] < 0) rs = fmin(rs, s[e][r] / -ds[r]);
          if (dz[r] < 0) rz = fmin(rz, z[e][r] / -dz[r]);
        }
      }
    const double al = fmin(1.0, 0.99 * fmin(rs, rz));
#pragma unroll
    for (int e = 0; e < NEE; ++e)
      if (Ft[e].on) {
        double ds[6], dz[6];
        qp_foot_step(Ft[e], mu, dx[e], s[e], z[e], t[e], ds, dz);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          s[e][r] = s[e][r] + al * ds[r];
          z[e][r] = z[e][r] + al * dz[r];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) x[e][i] = x[e][i] + al * dx[e][i];
      }
    ++steps;
  }
  return steps;
}
// objective(x) - objective(x_fit) as force_qp.objective_gap forms it, and |x - x_fit|^2 into dsq.
__device__ inline double qp_gap(const QpFoot Ft[NEE], const double rho[6], double c, const double xfit[NEE][3], const double x[NEE][3], double &dsq) {
#pragma clang fp contract(off)
  double g[NEE][3], AD[6] = {0, 0, 0, 0, 0, 0}, lin = 0, quad = 0;
  qp_grad(Ft, rho, c, xfit, g);
  dsq = 0;
#pragma unroll
  for (int e = 0; e < NEE; ++e)
    if (Ft[e].on) {
      const double D[3] = {x[e][0] - xfit[e][0], x[e][1] - xfit[e][1], x[e][2] - xfit[e][2]};
      const double *d = Ft[e].d;
      AD[0] = AD[0] + (d[1] * D[2] - d[2] * D[1]);
      AD[1] = AD[1] + (d[2] * D[0] - d[0] * D[2]);
      AD[2] = AD[2] + (d[0] * D[1] - d[1] * D[0]);
      AD[3] = AD[3] + D[0]; AD[4] = AD[4] + D[1]; AD[5] = AD[5] + D[2];
      lin = lin + qp_dot(g[e], D);
      const double dd = qp_dot(D, D);
      quad = quad + (c / Ft[e].w) * dd;
      dsq = dsq + dd;
    }
  const double sq = ((((AD[0] * AD[0] + AD[1] * AD[1]) + AD[2] * AD[2]) + AD[3] * AD[3]) + AD[4] * AD[4]) + AD[5] * AD[5];
  return lin + 0.5 * (sq + quad);
}
// A stance foot's df = x_e taken off the residual rows and added to the squared change (fit_foot_correct's lines, one rounded
// operation each, as force_qp.py forms them).
__device__ inline void qp_foot_residual(FitFoot &F, const double xe[3], double ra[3], double rl[3], double &sq) {
#pragma clang fp contract(off)
  if (!F.stance) return;
  F.df[0] = xe[0]; F.df[1] = xe[1]; F.df[2] = xe[2];
  ra[0] = ra[0] - (F.p[1] * xe[2] - F.p[2] * xe[1]);
  ra[1] = ra[1] - (F.p[2] * xe[0] - F.p[0] * xe[2]);
  ra[2] = ra[2] - (F.p[0] * xe[1] - F.p[1] * xe[0]);
  rl[0] = rl[0] - xe[0]; rl[1] = rl[1] - xe[1]; rl[2] = rl[2] - xe[2];
  sq = sq + ((xe[0] * xe[0] + xe[1] * xe[1]) + xe[2] * xe[2]);
}
__device__ inline void qp_foot_of(const FitFoot &F, double arm, QpFoot &Q, double xfit[3]) {
#pragma clang fp contract(off)
  Q.on = F.stance;
  Q.w = F.w;
#pragma unroll
  for (int i = 0; i < 3; ++i) { Q.d[i] = F.p[i] / arm; Q.f[i] = F.f[i]; xfit[i] = F.stance ? F.df[i] : 0.0; }
  qp_basis(F.hx, F.hy, Q.B);
}

__global__ __launch_bounds__(QP_TILE) void k_force_qp(const SamplePlan *Sd, FitArgs A, QpArgs Q, const double *nodes, const double *t0,
                                                      const int *map_id, const int *first_row, const int *n_rows, const long long *cursor,
                                                      const double *joint, const double *mass_scale, double *rows_out, double *qrows_out,
                                                      int *status_out, CheckRecord *summary, int B) {
  __shared__ double qp_slab[QP_SLAB * QP_TILE];
  __shared__ double qp_tile[QP_TILE * FIT_PITCH];
  __shared__ double qp_qtile[QP_TILE * QP_PITCH];
  __shared__ double qp_red[QP_TILE];
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long n = G.n, rows_b = G.rows_b;
  const long long row0 = A.capacity > 0 ? cursor[b] : G.first;                       // what the summary counts its rows from
  const int map = map_id ? map_id[b] : 0;
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  const double ms = mass_scale ? mass_scale[b] : 1.0;
  const double m_s = A.mass * ms;
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)rows_b * FIT_COLS : nullptr;
  double *qout_b = qrows_out ? qrows_out + (size_t)b * (size_t)rows_b * QP_COLS : nullptr;
  const double *joint_b = joint ? joint + (size_t)b * (size_t)rows_b * QTOS_CSV_COLS : nullptr;
  double run_max[FIT_FAMILIES];
  long long run_row[FIT_FAMILIES], run_cnt[FIT_FAMILIES];
#pragma unroll
  for (int f = 0; f < FIT_FAMILIES; ++f) { run_max[f] = -INFINITY; run_row[f] = -1; run_cnt[f] = 0; }
  for (long long j0 = 0; j0 < n; j0 += QP_TILE) {                                    // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, QP_TILE);
    const long long base = G.row(j0);
    double v[FIT_FAMILIES];
#pragma unroll
    for (int f = 0; f < FIT_FAMILIES; ++f) v[f] = -INFINITY;
    if ((int)threadIdx.x < m) {                                                      // (A) a lane takes a row: k_force_fit's lines up to the fit
      const int k = G.plan_row(j0, threadIdx.x);
      double t = k / A.hz;
      if (t > S.T) t = S.T;
      double *dst = qp_tile + threadIdx.x * FIT_PITCH;
      double *qdst = qp_qtile + threadIdx.x * QP_PITCH;
      dst[0] = t0b + k / A.hz;
      double r[3], a[3], th[3], thd[3], thdd[3], ga[3], gl[3], R[9], Ib[9];
      sample_spline(S.lin, x, t, 0, r);
      sample_spline_acc(S.lin, x, t, a);
      sample_spline(S.ang, x, t, 0, th);
      sample_spline(S.ang, x, t, 1, thd);
      sample_spline_acc(S.ang, x, t, thdd);
      const Trig tg = trig_of(th);
#pragma unroll
      for (int i = 0; i < 9; ++i) Ib[i] = ms * A.Ib[i];
      dyn_angular<double>(Ib, th, thd, thdd, tg, ga);
      rotation<double>(th, tg, R);
      gl[0] = m_s * a[0]; gl[1] = m_s * a[1]; gl[2] = m_s * a[2] + m_s * A.gravity;
      FitFoot F0, F1, F2, F3;
      fit_foot_load<0>(S, A, x, t, map, r, ga, gl, F0);
      fit_foot_load<1>(S, A, x, t, map, r, ga, gl, F1);
      fit_foot_load<2>(S, A, x, t, map, r, ga, gl, F2);
      fit_foot_load<3>(S, A, x, t, map, r, ga, gl, F3);
      const int cnt = (int)F0.stance + (int)F1.stance + (int)F2.stance + (int)F3.stance;
      const double nn = (double)cnt, gsum = ((F0.w + F1.w) + F2.w) + F3.w;
      const bool loaded = gsum > 0;
      F0.w = loaded ? fmax(nn * F0.w / gsum, A.w_min) : 1.0;
      F1.w = loaded ? fmax(nn * F1.w / gsum, A.w_min) : 1.0;
      F2.w = loaded ? fmax(nn * F2.w / gsum, A.w_min) : 1.0;
      F3.w = loaded ? fmax(nn * F3.w / gsum, A.w_min) : 1.0;
      const double rho_w[6] = {ga[0], ga[1], ga[2], gl[0], gl[1], gl[2]};            // the plan's own dynamics rows
      const double rho[6] = {ga[0] / A.arm, ga[1] / A.arm, ga[2] / A.arm, gl[0], gl[1], gl[2]};
      double y[6] = {0, 0, 0, 0, 0, 0}, sq = 0;
      if (cnt > 0) {
        FitSums Qs = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        fit_foot_sums(F0, A.arm, Qs);
        fit_foot_sums(F1, A.arm, Qs);
        fit_foot_sums(F2, A.arm, Qs);
        fit_foot_sums(F3, A.arm, Qs);
        const double lam = A.damping * nn, wl = Qs.W + lam;
        double M[21] = {(Qs.q11 + Qs.q22) + lam,
                        -Qs.q01, (Qs.q00 + Qs.q22) + lam,
                        -Qs.q02, -Qs.q12, (Qs.q00 + Qs.q11) + lam,
                        0.0, Qs.s2, -Qs.s1, wl,
                        -Qs.s2, 0.0, Qs.s0, 0.0, wl,
                        Qs.s1, -Qs.s0, 0.0, 0.0, 0.0, wl};
        fit_solve<FitExact>(M, rho, y);
      }
      fit_foot_correct(F0, A.arm, y, ga, gl, sq);
      fit_foot_correct(F1, A.arm, y, ga, gl, sq);
      fit_foot_correct(F2, A.arm, y, ga, gl, sq);
      fit_foot_correct(F3, A.arm, y, ga, gl, sq);
      double change = sqrt(sq);
      bool fin = isfinite(ga[0]) && isfinite(ga[1]) && isfinite(ga[2]) && isfinite(gl[0]) && isfinite(gl[1]) && isfinite(gl[2]) &&
                 isfinite(change);
      fin = fin && isfinite(F0.df[0]) && isfinite(F0.df[1]) && isfinite(F0.df[2]) && isfinite(F1.df[0]) && isfinite(F1.df[1]) &&
            isfinite(F1.df[2]) && isfinite(F2.df[0]) && isfinite(F2.df[1]) && isfinite(F2.df[2]) && isfinite(F3.df[0]) &&
            isfinite(F3.df[1]) && isfinite(F3.df[2]);
      bool bad = !fin;
      // the limits on the fit's forces: the slacks h - G (f + df_fit) of the stance feet
      QpFoot Ft[NEE];
      double xfit[NEE][3], sl[NEE][6], zl[NEE][6], xq[NEE][3];
      qp_foot_of(F0, A.arm, Ft[0], xfit[0]);
      qp_foot_of(F1, A.arm, Ft[1], xfit[1]);
      qp_foot_of(F2, A.arm, Ft[2], xfit[2]);
      qp_foot_of(F3, A.arm, Ft[3], xfit[3]);
      bool inside = true;
#pragma unroll
      for (int e = 0; e < NEE; ++e) {
#pragma unroll
        for (int q6 = 0; q6 < 6; ++q6) { sl[e][q6] = NAN; zl[e][q6] = 0.0; }
        if (Ft[e].on) {
          const double ff[3] = {Ft[e].f[0] + xfit[e][0], Ft[e].f[1] + xfit[e][1], Ft[e].f[2] + xfit[e][2]};
          double gv[6];
          qp_gmul(Ft[e].B, Q.mu, ff, gv);
#pragma unroll
          for (int q6 = 0; q6 < 6; ++q6) {
            const double val = gv[q6] - (q6 == 1 ? Q.f_max : 0.0);
            if (!(val <= 0)) inside = false;
            sl[e][q6] = -val;
          }
        }
      }
      const bool limited = cnt > 0 && !bad && !inside;
      double qcol[QP_COLS] = {0, 0, 0, 0, 0, 0, 0, 0};
      bool cap = false;
      if (limited) {
        double comp, rdn, dsq;
        const int steps = qp_solve(Ft, rho, A.damping * nn, 6.0 * nn, Q, xfit, qp_slab + threadIdx.x, xq, sl, zl, comp, rdn, cap);
        ga[0] = rho_w[0]; ga[1] = rho_w[1]; ga[2] = rho_w[2]; gl[0] = rho_w[3]; gl[1] = rho_w[4]; gl[2] = rho_w[5];
        sq = 0;
        qp_foot_residual(F0, xq[0], ga, gl, sq);
        qp_foot_residual(F1, xq[1], ga, gl, sq);
        qp_foot_residual(F2, xq[2], ga, gl, sq);
        qp_foot_residual(F3, xq[3], ga, gl, sq);
        change = sqrt(sq);
        const double gap = qp_gap(Ft, rho, A.damping * nn, xfit, xq, dsq);
        bool f2 = isfinite(ga[0]) && isfinite(ga[1]) && isfinite(ga[2]) && isfinite(gl[0]) && isfinite(gl[1]) && isfinite(gl[2]) && isfinite(change);
#pragma unroll
        for (int e = 0; e < NEE; ++e) f2 = f2 && isfinite(xq[e][0]) && isfinite(xq[e][1]) && isfinite(xq[e][2]);
        bad = !f2;
        double smin = INFINITY, zmax = 0;
#pragma unroll
        for (int e = 0; e < NEE; ++e)
          if (Ft[e].on) {
#pragma unroll
            for (int q6 = 0; q6 < 6; ++q6) { smin = fmin(smin, sl[e][q6]); zmax = fmax(zmax, zl[e][q6]); }
          }
        qcol[0] = (double)steps;
        qcol[1] = bad ? NAN : comp; qcol[2] = bad ? NAN : rdn; qcol[3] = bad ? NAN : smin; qcol[4] = bad ? NAN : zmax;
        qcol[5] = bad ? NAN : sqrt(dsq); qcol[6] = bad ? NAN : gap;
      } else if (cnt > 0 && !bad) {
        double smin = INFINITY;
#pragma unroll
        for (int e = 0; e < NEE; ++e)
          if (Ft[e].on) {
#pragma unroll
            for (int q6 = 0; q6 < 6; ++q6) smin = fmin(smin, sl[e][q6]);
          }
        qcol[3] = smin;
      } else if (bad) {
#pragma unroll
        for (int c6 = 1; c6 < 7; ++c6) qcol[c6] = NAN;
      }
      dst[13] = bad ? NAN : ga[0]; dst[14] = bad ? NAN : ga[1]; dst[15] = bad ? NAN : ga[2];
      dst[16] = bad ? NAN : gl[0]; dst[17] = bad ? NAN : gl[1]; dst[18] = bad ? NAN : gl[2];
      dst[19] = bad ? NAN : change;
      const double *q = joint_b ? joint_b + (size_t)G.tile_row(base, threadIdx.x) * QTOS_CSV_COLS + 1 : nullptr;
      double v_ex = 0;
      fit_foot_out<0>(A, F0, bad, R, q, dst, v_ex);                                  // (the forces and the torques; its excess bits are not this kernel's)
      fit_foot_out<1>(A, F1, bad, R, q, dst, v_ex);
      fit_foot_out<2>(A, F2, bad, R, q, dst, v_ex);
      fit_foot_out<3>(A, F3, bad, R, q, dst, v_ex);
      int st = (cnt == 0 ? 1 : 0) | (cnt == 2 ? 2 : 0) | (bad ? 4 : 0) | (limited ? 256 : 0) | (cap ? 128 : 0);
      int n_act = 0;
#pragma unroll
      for (int e = 0; e < NEE; ++e)
        if (Ft[e].on && !bad) {
#pragma unroll
          for (int q6 = 0; q6 < 6; ++q6)
            if (sl[e][q6] <= Q.act_tol) { ++n_act; st |= 8 << e; }
        }
      qcol[7] = (double)n_act;
#pragma unroll
      for (int c6 = 0; c6 < QP_COLS; ++c6) qdst[c6] = qcol[c6];
      if (status_out) status_out[(size_t)b * (size_t)rows_b + G.tile_row(base, threadIdx.x)] = st;
      v[0] = bad ? INFINITY : fmax(fmax(fabs(ga[0]), fabs(ga[1])), fabs(ga[2]));
      v[1] = bad ? INFINITY : fmax(fmax(fabs(gl[0]), fabs(gl[1])), fabs(gl[2]));
      v[2] = bad ? INFINITY : change;
      v[3] = isfinite(qcol[5]) ? fabs(qcol[5]) : INFINITY;
    }
    if (summary) {                                                                   // (B) the tile's families into the running records
#pragma unroll
      for (int f = 0; f < FIT_FAMILIES; ++f) {
        const double mx = wg_reduce<1, QP_TILE>(v[f], qp_red);
        const double at = wg_reduce<2, QP_TILE>(v[f] == mx ? (double)threadIdx.x : (double)QP_TILE, qp_red);
        const double over = wg_reduce<0, QP_TILE>(v[f] > A.tol[f] ? 1.0 : 0.0, qp_red);
        if (mx > run_max[f]) { run_max[f] = mx; run_row[f] = row0 + j0 + (long long)at; }
        run_cnt[f] += (long long)over;
      }
    }
    __syncthreads();
    if (out_b) {                                                                     // (C) the tiles go out flat
      for (int e = threadIdx.x; e < m * FIT_COLS; e += QP_TILE) {
        const int i = e / FIT_COLS, c = e - i * FIT_COLS;
        if (c < 20 || joint_b) out_b[G.flat(base, FIT_COLS, e)] = qp_tile[i * FIT_PITCH + c];
      }
    }
    if (qout_b) {
      for (int e = threadIdx.x; e < m * QP_COLS; e += QP_TILE) {
        const int i = e / QP_COLS, c = e - i * QP_COLS;
        qout_b[G.flat(base, QP_COLS, e)] = qp_qtile[i * QP_PITCH + c];
      }
    }
    __syncthreads();
  }
  if (summary && threadIdx.x == 0) {
    if (A.accumulate && n == 0) return;
#pragma unroll
    for (int f = 0; f < FIT_FAMILIES; ++f) {
      CheckRecord rec = {run_max[f], run_row[f], run_cnt[f]};
      CheckRecord *dst = summary + (size_t)b * FIT_FAMILIES + f;
      if (A.accumulate) {
        const CheckRecord old = *dst;
        if (!(rec.max > old.max)) { rec.max = old.max; rec.row = old.row; }
        rec.count += old.count;
      }
      *dst = rec;
    }
  }
}

// Rollout through the feet (qtos_rollout_feet*): k_rollout with its feedback wrench delivered by the feet that stand.  The
// statement of the rule is rollout_feet.py: lines 1, 2, 4 .. 7 and 9 .. 11 of the step are k_rollout's (rollout_feedback,
// rollout_advance), lines 3 and 8 are replaced -- the clipped PD wrench is distributed over the stance feet by k_force_fit's damped
// load-weighted 6 x 6 solve (its ten sums, its matrix and fit_solve, here with one rounded operation per operation), the forces
// act at the plan's footholds about the ACTUAL centre of mass and, with QTOS_FEET_LIMIT, are limited by comparisons to what a
// foot can do.  The kernel has k_rollout's shape: one workgroup per window; per tile (A) a lane takes a row -- the plan row, the
// 20 inputs, the feet's positions and forces, the load weights from the forces' vertical components and the stance mask into the
// row's place of an LDS tile; (B) lane 0 walks the chain, only +, -, x, / and sqrt, the 21 entries of M and of L in registers with
// constant indices (the feet come through unrolled loops); the applied forces and the missing wrench of a tick's FIRST step stay
// in registers until the tick's last step has read the plan's forces, then take their place; (C) a lane turns its row's state into
// the output columns, and the tile goes out flat: rows, meas and the 16-column feet rows (RowSegment's addressing).
// A row of the tile, FEET_PITCH = 67 doubles (odd: consecutive lanes on different banks): 0 .. 19 the inputs / outputs, 20 .. 31
// p_e, 32 .. 43 f_e (behind the tick: f_a), 44 .. 47 w_e (behind the tick: columns 13 .. 15), 48 the stance mask, 49 .. 61 the
// state, 62 |e|, 63 tilt, 64 |F_fb|, 65 the status, 66 unused.  256 x 67 x 8 = 137 216 bytes of LDS, 64 x 67 x 8 = 34 304 for
// the tick.  No atomics, no scratch, every barrier uniform.
constexpr int FEET_COLS = 16;
constexpr int FEET_PITCH = 67;
constexpr int ROLLQP_PITCH = 75, ROLLQP_Q = 67;              // k_rollout_qp's row (below): the solve's 8 columns behind the feet's places
constexpr int FEET_P = 20, FEET_F = 32, FEET_W = 44, FEET_MASK = 48, FEET_STATE = 49, FEET_STATUS = 65;   // places in a row of the tile
struct FeetArgs {   // QtosRolloutFeet's own fields as the kernel reads them (window_api.hpp rollout_feet_args)
  double arm, damping, w_min, mu, f_max;
  const int *stance[NEE];                  // per foot and polynomial of its motion spline: 1 stance, 0 swing
  int limit;
};
struct FeetOut { double fa[12], miss_f, miss_t, change; };   // columns 1 .. 15 of a feet row
// What a step of the rollout with the force QP (k_rollout_qp, below) adds: the solve's eight columns, its two bits, and where the
// chain lane keeps K and the solves' vector -- 90 doubles of LDS at stride 1.
struct FeetQp {
  const QpArgs *Q;
  double *slab;
  double col[QP_COLS];
  bool limited, cap;
};

// The feet of a plan row c (37 columns) into the row's place d of the tile: p_e, f_e, the load weights w_e from the vertical
// components of the stance feet's forces and the stance mask (rollout_feet.plan_feet).
__device__ inline void feet_inputs(const double *c, int mask, double w_min, double *d) {
#pragma clang fp contract(off)
  double g[NEE];
  int cnt = 0;
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    const bool on = (mask >> e) & 1;
#pragma unroll
    for (int i = 0; i < 3; ++i) { d[FEET_P + 3 * e + i] = c[7 + 3 * e + i]; d[FEET_F + 3 * e + i] = c[25 + 3 * e + i]; }
    const double fz = c[27 + 3 * e];
    g[e] = on && fz > 0 ? fz : 0.0;
    cnt += on ? 1 : 0;
  }
  const double gsum = ((g[0] + g[1]) + g[2]) + g[3], nn = (double)cnt;
  const bool loaded = gsum > 0;
#pragma unroll
  for (int e = 0; e < NEE; ++e) {
    const double x = (nn * g[e]) / gsum;
    d[FEET_W + e] = loaded ? (x < w_min ? w_min : x) : 1.0;
  }
  d[FEET_MASK] = (double)mask;
}

// One step of length A.h under the row p of the tile (rollout_feet.step); returns |F_fb|.  o: the applied forces and what the
// feet did not deliver, of this step.  QP (rollout_qp.step, k_rollout_qp): the stance forces are the fit's where those lie inside
// the limits and the central point of force_qp.py's barrier problem where they do not, in place of the comparisons; qp: the
// solve's columns and bits of this step.
template <bool QP = false>
__device__ inline double rollout_feet_step(const RolloutArgs &A, const FeetArgs &Ft, const RolloutBody &M, const double *p, bool push,
                                           RolloutState &s, bool &clipped, bool &limited, FeetOut &o, FeetQp *qp = nullptr) {
#pragma clang fp contract(off)
  double e[3], b[3], R[9], c[3];
  rollout_feedback(A, p, s, e, b, R, c, clipped);
  const double arm = Ft.arm, ff = A.ff_scale;
  const double rhs[6] = {c[0] / arm, c[1] / arm, c[2] / arm, b[0], b[1], b[2]};
  const int mask = (int)p[FEET_MASK];
  double l[12], d[12];
  FitSums Q = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < NEE; ++k) {
    l[3 * k] = p[FEET_P + 3 * k] - s.r0; l[3 * k + 1] = p[FEET_P + 3 * k + 1] - s.r1; l[3 * k + 2] = p[FEET_P + 3 * k + 2] - s.r2;
    d[3 * k] = l[3 * k] / arm; d[3 * k + 1] = l[3 * k + 1] / arm; d[3 * k + 2] = l[3 * k + 2] / arm;
    if ((mask >> k) & 1) {                                     // fit_foot_sums' lines, one rounded operation each
      const double w = p[FEET_W + k];
      const double w0 = w * d[3 * k], w1 = w * d[3 * k + 1], w2 = w * d[3 * k + 2];
      Q.W = Q.W + w; Q.s0 = Q.s0 + w0; Q.s1 = Q.s1 + w1; Q.s2 = Q.s2 + w2;
      Q.q00 = Q.q00 + w0 * d[3 * k]; Q.q01 = Q.q01 + w0 * d[3 * k + 1]; Q.q02 = Q.q02 + w0 * d[3 * k + 2];
      Q.q11 = Q.q11 + w1 * d[3 * k + 1]; Q.q12 = Q.q12 + w1 * d[3 * k + 2]; Q.q22 = Q.q22 + w2 * d[3 * k + 2];
      ++cnt;
    }
  }
  double y[6] = {0, 0, 0, 0, 0, 0};
  if (cnt > 0) {
    const double lam = Ft.damping * (double)cnt, wl = Q.W + lam;
    double K[21] = {(Q.q11 + Q.q22) + lam,
                    -Q.q01, (Q.q00 + Q.q22) + lam,
                    -Q.q02, -Q.q12, (Q.q00 + Q.q11) + lam,
                    0.0, Q.s2, -Q.s1, wl,
                    -Q.s2, 0.0, Q.s0, 0.0, wl,
                    Q.s1, -Q.s0, 0.0, 0.0, 0.0, wl};
    fit_solve<FitExact>(K, rhs, y);
  }
  double Fa[3] = {0, 0, 0}, ta[3] = {0, 0, 0}, gF[3] = {0, 0, 0}, gT[3] = {0, 0, 0}, sq = 0;
  [[maybe_unused]] double xq[NEE][3];
  [[maybe_unused]] bool qp_path = false;
  if constexpr (QP) {                                          // the path and, on the limited one, the QP's x in place of df
    const QpArgs &Qa = *qp->Q;
    QpFoot Fq[NEE];
    double xfit[NEE][3], sl[NEE][6], zl[NEE][6];
    bool inside = true;
#pragma unroll
    for (int k = 0; k < NEE; ++k) {
      const double *dk = d + 3 * k;
      QpFoot &F = Fq[k];
      F.on = (mask >> k) & 1;
      F.w = p[FEET_W + k];
      F.d[0] = dk[0]; F.d[1] = dk[1]; F.d[2] = dk[2];
      F.f[0] = ff * p[FEET_F + 3 * k]; F.f[1] = ff * p[FEET_F + 3 * k + 1]; F.f[2] = ff * p[FEET_F + 3 * k + 2];
      qp_basis(0.0, 0.0, F.B);                                 // (the rollout reads no terrain)
      xfit[k][0] = 0; xfit[k][1] = 0; xfit[k][2] = 0;
#pragma unroll
      for (int r = 0; r < 6; ++r) { sl[k][r] = NAN; zl[k][r] = 0.0; }
      if (F.on) {
        xfit[k][0] = ((y[1] * dk[2] - y[2] * dk[1]) + y[3]) * F.w;
        xfit[k][1] = ((y[2] * dk[0] - y[0] * dk[2]) + y[4]) * F.w;
        xfit[k][2] = ((y[0] * dk[1] - y[1] * dk[0]) + y[5]) * F.w;
        const double fit[3] = {F.f[0] + xfit[k][0], F.f[1] + xfit[k][1], F.f[2] + xfit[k][2]};
        double gv[6];
        qp_gmul(F.B, Qa.mu, fit, gv);
#pragma unroll
        for (int r = 0; r < 6; ++r) {
          const double val = gv[r] - (r == 1 ? Qa.f_max : 0.0);
          if (!(val <= 0)) inside = false;                     // (a NaN takes the limited path and runs into the cap)
          sl[k][r] = -val;
        }
      }
    }
    qp_path = cnt > 0 && !inside;
#pragma unroll
    for (int c = 0; c < QP_COLS; ++c) qp->col[c] = 0.0;
    qp->limited = qp_path; qp->cap = false;
    if (qp_path) {
      double comp, rdn, dsq;
      const double cq = Ft.damping * (double)cnt;
      const int steps = qp_solve<1>(Fq, rhs, cq, 6.0 * (double)cnt, Qa, xfit, qp->slab, xq, sl, zl, comp, rdn, qp->cap);
      const double gap = qp_gap(Fq, rhs, cq, xfit, xq, dsq);
      qp->col[0] = (double)steps; qp->col[1] = comp; qp->col[2] = rdn; qp->col[5] = sqrt(dsq); qp->col[6] = gap;
    }
    if (cnt > 0) {
      double smin = INFINITY, zmax = 0;
      int n_act = 0;
#pragma unroll
      for (int k = 0; k < NEE; ++k)
        if (Fq[k].on) {
#pragma unroll
          for (int r = 0; r < 6; ++r) {
            smin = sl[k][r] < smin ? sl[k][r] : smin;          // (by comparisons: numpy's min; a NaN is not taken here, the
            zmax = zl[k][r] > zmax ? zl[k][r] : zmax;          //  row it belongs to ends at the cap and is frozen behind it)
            if (sl[k][r] <= Qa.act_tol) ++n_act;
          }
        }
      qp->col[3] = smin; qp->col[7] = (double)n_act;
      if (qp_path) qp->col[4] = zmax;
    }
    limited = limited || qp_path;
  }
#pragma unroll
  for (int k = 0; k < NEE; ++k) {
    const bool on = (mask >> k) & 1;
    const double *dk = d + 3 * k, *lk = l + 3 * k;
    const double f0 = ff * p[FEET_F + 3 * k], f1 = ff * p[FEET_F + 3 * k + 1], f2 = ff * p[FEET_F + 3 * k + 2];
    double a0 = f0 + 0.0, a1 = f1 + 0.0, a2 = f2 + 0.0;
    if (on) {
      const double w = p[FEET_W + k];
      a0 = f0 + ((y[1] * dk[2] - y[2] * dk[1]) + y[3]) * w;
      a1 = f1 + ((y[2] * dk[0] - y[0] * dk[2]) + y[4]) * w;
      a2 = f2 + ((y[0] * dk[1] - y[1] * dk[0]) + y[5]) * w;
      if constexpr (QP) {
        if (qp_path) { a0 = f0 + xq[k][0]; a1 = f1 + xq[k][1]; a2 = f2 + xq[k][2]; }
      } else if (Ft.limit) {                                   // by comparisons only: a NaN stays a NaN
        if (a2 < 0) { a2 = 0.0; limited = true; }
        if (Ft.f_max > 0 && a2 > Ft.f_max) { a2 = Ft.f_max; limited = true; }
        const double lim = Ft.mu * a2;
        if (a0 < -lim) { a0 = -lim; limited = true; } else if (a0 > lim) { a0 = lim; limited = true; }
        if (a1 < -lim) { a1 = -lim; limited = true; } else if (a1 > lim) { a1 = lim; limited = true; }
      }
    }
    o.fa[3 * k] = a0; o.fa[3 * k + 1] = a1; o.fa[3 * k + 2] = a2;
    const double x0 = lk[1] * a2 - lk[2] * a1, x1 = lk[2] * a0 - lk[0] * a2, x2 = lk[0] * a1 - lk[1] * a0;
    if (k == 0) { Fa[0] = a0; Fa[1] = a1; Fa[2] = a2; ta[0] = x0; ta[1] = x1; ta[2] = x2; }
    else { Fa[0] = Fa[0] + a0; Fa[1] = Fa[1] + a1; Fa[2] = Fa[2] + a2; ta[0] = ta[0] + x0; ta[1] = ta[1] + x1; ta[2] = ta[2] + x2; }
    if (on) {                                                  // what this foot adds to the plan's force, and its moment
      const double g0 = a0 - f0, g1 = a1 - f1, g2 = a2 - f2;
      gF[0] = gF[0] + g0; gF[1] = gF[1] + g1; gF[2] = gF[2] + g2;
      gT[0] = gT[0] + (lk[1] * g2 - lk[2] * g1); gT[1] = gT[1] + (lk[2] * g0 - lk[0] * g2); gT[2] = gT[2] + (lk[0] * g1 - lk[1] * g0);
      sq = sq + ((g0 * g0 + g1 * g1) + g2 * g2);
    }
  }
  o.miss_f = rollout_norm(gF[0] - b[0], gF[1] - b[1], gF[2] - b[2]);
  o.miss_t = rollout_norm(gT[0] - c[0], gT[1] - c[1], gT[2] - c[2]);
  o.change = sqrt(sq);
  const double P0 = push ? M.F0 : 0.0, P1 = push ? M.F1 : 0.0, P2 = push ? M.F2 : 0.0;
  const double Q0 = push ? M.T0 : 0.0, Q1 = push ? M.T1 : 0.0, Q2 = push ? M.T2 : 0.0;
  const double a[3] = {(Fa[0] + P0) / M.m_s, (Fa[1] + P1) / M.m_s, (Fa[2] + P2) / M.m_s - A.gravity};
  const double t[3] = {ta[0] + Q0, ta[1] + Q1, ta[2] + Q2};
  rollout_advance(A, M, R, a, t, s);
  return rollout_norm(b[0], b[1], b[2]);
}

// (k_rollout_qp, below, carries a twin of this kernel's text -- INIT / PENDING, the freeze, phases (A) and (C), the write-out --
// with its own pitch, step and solve table: a change here belongs there too.)
template <int TILE>
__global__ __launch_bounds__(TILE) void k_rollout_feet(const SamplePlan *Sd, RolloutArgs A, FeetArgs Ft, const double *nodes, const double *t0,
                                                       const int *first_row, const int *n_rows, const long long *cursor,
                                                       const double *joint, const double *mass_scale, const double *push, double *state,
                                                       long long *count, int *word_io, double *meas, double *rows_out, double *frows_out,
                                                       int *status_out, int B) {
  __shared__ double feet_tile[TILE * FEET_PITCH];
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const bool quat = (A.flags & 2) != 0;
  const int mcols = quat ? 19 : 18;
  RolloutState s;                                                                  // (every lane, in front of the first barrier)
  {
    const double *sb = state + (size_t)b * 13;
    s.r0 = sb[0]; s.r1 = sb[1]; s.r2 = sb[2]; s.v0 = sb[3]; s.v1 = sb[4]; s.v2 = sb[5];
    s.qx = sb[6]; s.qy = sb[7]; s.qz = sb[8]; s.qw = sb[9]; s.w0 = sb[10]; s.w1 = sb[11]; s.w2 = sb[12];
  }
  const long long calls = count[b];
  int word = word_io[b];
  RolloutBody M;
  {
#pragma clang fp contract(off)
    const double ms = mass_scale ? mass_scale[b] : 1.0;
    M.m_s = A.mass * ms;
#pragma unroll
    for (int i = 0; i < 9; ++i) { M.I[i] = ms * A.Ib[i]; M.J[i] = A.Ii[i] / ms; }
    const double *pb = push ? push + (size_t)b * 6 : nullptr;
    M.F0 = pb ? pb[0] : 0.0; M.F1 = pb ? pb[1] : 0.0; M.F2 = pb ? pb[2] : 0.0;
    M.T0 = pb ? pb[3] : 0.0; M.T1 = pb ? pb[4] : 0.0; M.T2 = pb ? pb[5] : 0.0;
  }
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long rows_b = G.rows_b, n = G.n;
  if (n == 0) return;                                                              // (uniform: a window without rows keeps its state)
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  double *meas_b = meas + (size_t)b * (size_t)rows_b * mcols;
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)rows_b * ROLLOUT_COLS : nullptr;
  double *feet_b = frows_out ? frows_out + (size_t)b * (size_t)rows_b * FEET_COLS : nullptr;
  const double *joint_b = joint ? joint + (size_t)b * (size_t)rows_b * QTOS_CSV_COLS : nullptr;
  for (long long j0 = 0; j0 < n; j0 += TILE) {                                     // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, TILE);
    const long long base = G.row(j0);
    if ((int)threadIdx.x < m) {                                                    // (A) a lane takes a row of the plan
      double row[QTOS_CSV_COLS];
      const double t = sample_row_state_at(S, x, t0b, G.plan_row(j0, threadIdx.x), A.hz, row);
      int mask = 0;
#pragma unroll
      for (int e = 0; e < NEE; ++e) {
        sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
        mask |= (Ft.stance[e][sample_segment(S.eem[e], t)] != 0 ? 1 : 0) << e;
      }
      double *dst = feet_tile + threadIdx.x * FEET_PITCH;
      rollout_inputs(row, A.ff_scale, dst);
      feet_inputs(row, mask, Ft.w_min, dst);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                        // (B) the chain, in program order
#pragma clang fp contract(off)
      if (j0 == 0 && ((A.flags & 1) || (word & 32))) {                             // QTOS_ROLLOUT_INIT / _PENDING, as in k_rollout
        word &= ~32;
        const double *p = feet_tile;
        s.r0 = p[1]; s.r1 = p[2]; s.r2 = p[3]; s.v0 = p[4]; s.v1 = p[5]; s.v2 = p[6];
        s.qx = p[7]; s.qy = p[8]; s.qz = p[9]; s.qw = p[10];
        const double qx = s.qx, qy = s.qy, qz = s.qz, qw = s.qw;
        const double R0 = 1 - 2 * (qy * qy + qz * qz), R1 = 2 * (qx * qy - qz * qw), R2 = 2 * (qx * qz + qy * qw);
        const double R3 = 2 * (qx * qy + qz * qw), R4 = 1 - 2 * (qx * qx + qz * qz), R5 = 2 * (qy * qz - qx * qw);
        const double R6 = 2 * (qx * qz - qy * qw), R7 = 2 * (qy * qz + qx * qw), R8 = 1 - 2 * (qx * qx + qy * qy);
        s.w0 = (R0 * p[11] + R3 * p[12]) + R6 * p[13];
        s.w1 = (R1 * p[11] + R4 * p[12]) + R7 * p[13];
        s.w2 = (R2 * p[11] + R5 * p[12]) + R8 * p[13];
      }
      for (int i = 0; i < m; ++i) {
        double *p = feet_tile + i * FEET_PITCH;
        double ex, ey, ez, ew;
        rollout_attitude(p, s, ex, ey, ez, ew);
        const double en = rollout_norm(s.r0 - p[1], s.r1 - p[2], s.r2 - p[3]);
        const double tilt = 2 * rollout_norm(ex, ey, ez);
        const bool finite = isfinite(s.r0) && isfinite(s.r1) && isfinite(s.r2) && isfinite(s.v0) && isfinite(s.v1) && isfinite(s.v2) &&
                            isfinite(s.qx) && isfinite(s.qy) && isfinite(s.qz) && isfinite(s.qw) && isfinite(s.w0) && isfinite(s.w1) &&
                            isfinite(s.w2);
        if (!finite) word |= 2;
        if ((A.dev_max > 0 && en > A.dev_max) || (A.tilt_max > 0 && tilt > A.tilt_max)) word |= 1;
        int st = word & 3;
        double *q = p + FEET_STATE;
        q[0] = s.r0; q[1] = s.r1; q[2] = s.r2; q[3] = s.v0; q[4] = s.v1; q[5] = s.v2;
        q[6] = s.qx; q[7] = s.qy; q[8] = s.qz; q[9] = s.qw; q[10] = s.w0; q[11] = s.w1; q[12] = s.w2;
        q[13] = en; q[14] = tilt;
        const int mask = (int)p[FEET_MASK];
        const int cnt = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
        const int feet_bits = (cnt == 0 ? 64 : 0) | (cnt == 2 ? 128 : 0);
        double fbn = 0;
        if (!st) {
          const long long c = calls + j0 + i;
          const bool acts = push != nullptr && c >= A.push_from && c - A.push_from < A.push_ticks;
          bool clipped = false, limited = false;
          FeetOut first;
          fbn = rollout_feet_step(A, Ft, M, p, acts, s, clipped, limited, first);
          for (int u = 1; u < A.substeps; ++u) {
            FeetOut later;
            rollout_feet_step(A, Ft, M, p, acts, s, clipped, limited, later);
          }
#pragma unroll
          for (int k = 0; k < 12; ++k) p[FEET_F + k] = first.fa[k];               // (behind the tick's last step: it read f_e and w_e)
          p[FEET_W] = first.miss_f; p[FEET_W + 1] = first.miss_t; p[FEET_W + 2] = first.change;
          st = (clipped ? 8 : 0) | (acts ? 16 : 0) | (limited ? 256 : 0);
        } else {
          p[FEET_W] = 0.0; p[FEET_W + 1] = 0.0; p[FEET_W + 2] = 0.0;             // a frozen row: the plan's forces stay in their place
        }
        q[15] = fbn; p[FEET_STATUS] = (double)(st | feet_bits);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < m) {                                                    // (C) a lane turns its row's state into the output columns
      double *p = feet_tile + threadIdx.x * FEET_PITCH;
      const int st = (int)p[FEET_STATUS] | rollout_output<FEET_STATE>(p);
      status_out[(size_t)b * (size_t)rows_b + G.tile_row(base, threadIdx.x)] = st;
    }
    __syncthreads();
    if (out_b) {                                                                   // the tile goes out flat: rows ...
      for (int e = threadIdx.x; e < m * ROLLOUT_COLS; e += TILE) {
        const int i = e / ROLLOUT_COLS, c = e - i * ROLLOUT_COLS;
        out_b[G.flat(base, ROLLOUT_COLS, e)] = feet_tile[i * FEET_PITCH + c];
      }
    }
    if (feet_b) {                                                                  // ... the feet rows ...
      for (int e = threadIdx.x; e < m * FEET_COLS; e += TILE) {
        const int i = e / FEET_COLS, c = e - i * FEET_COLS;
        const double *p = feet_tile + i * FEET_PITCH;
        feet_b[G.flat(base, FEET_COLS, e)] = c == 0 ? p[0] : (c < 13 ? p[FEET_F + (c - 1)] : p[FEET_W + (c - 13)]);
      }
    }
    for (int e = threadIdx.x; e < m * mcols; e += TILE) {                          // ... and meas
      const int i = e / mcols, c = e - i * mcols;
      const double *p = feet_tile + i * FEET_PITCH;
      const long long o = G.flat(base, mcols, e);
      if (c < 3) meas_b[o] = p[1 + c];
      else if (c < mcols - 12) meas_b[o] = quat ? p[13 + (c - 3)] : p[4 + (c - 3)];
      else if (joint_b) meas_b[o] = joint_b[(size_t)G.tile_row(base, i) * QTOS_CSV_COLS + 1 + (c - (mcols - 12))];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *sb = state + (size_t)b * 13;
    sb[0] = s.r0; sb[1] = s.r1; sb[2] = s.r2; sb[3] = s.v0; sb[4] = s.v1; sb[5] = s.v2;
    sb[6] = s.qx; sb[7] = s.qy; sb[8] = s.qz; sb[9] = s.qw; sb[10] = s.w0; sb[11] = s.w1; sb[12] = s.w2;
    count[b] = calls + n;
    word_io[b] = word;
  }
}

// Rollout with the force QP (qtos_rollout_qp*; the rule: rollout_qp.py): k_rollout_feet with k_force_qp's limited path in place of
// its comparisons, in every step of the chain.  The phases (A), (B), (C) and the flat write-out are k_rollout_feet's; the chain on
// lane 0 reuses rollout_feedback, rollout_advance, fit_solve<FitExact> and the qp_* functions (one copy of each: the iteration is
// k_force_qp's, instantiated at stride 1 on a slab of the chain lane's own, QP_SLAB = 90 doubles).  A row of the tile grows by the
// solve's 8 columns of the tick's first step, places 67 .. 74: ROLLQP_PITCH = 75 doubles (odd, as FEET_PITCH is), so 256 x 75 x 8 +
// 720 = 154 320 bytes of LDS for the table's instantiation, under the 160 KB of a gfx950 workgroup, and 64 x 75 x 8 + 720 = 39 120
// for the tick's.  Contraction is off in every function of the chain; every loop has a fixed bound (at most QP_MAX_ITER steps of
// 12 columns); no atomics; every barrier uniform.  The lanes beside the chain wait at the barrier: a tick costs the chain's latency
// on one lane, one f64 operation after the other.  The text below is k_rollout_feet's but for the pitch, the step and the solve's
// table (a body shared by both kernels changed k_rollout_feet's register allocation): a change to one belongs
// in the other.
template <int TILE>
__global__ __launch_bounds__(TILE) void k_rollout_qp(const SamplePlan *Sd, RolloutArgs A, FeetArgs Ft, QpArgs Q, const double *nodes,
                                                     const double *t0, const int *first_row, const int *n_rows, const long long *cursor,
                                                     const double *joint, const double *mass_scale, const double *push, double *state,
                                                     long long *count, int *word_io, double *meas, double *rows_out, double *frows_out,
                                                     double *qrows_out, int *status_out, int B) {
  __shared__ double rollqp_tile[TILE * ROLLQP_PITCH];
  __shared__ double rollqp_slab[QP_SLAB];                                           // (K and the solves' vector of the chain lane, at stride 1)
  const int b = blockIdx.x;
  if (b >= B) return;
  const SamplePlan &S = *Sd;
  const bool quat = (A.flags & 2) != 0;
  const int mcols = quat ? 19 : 18;
  RolloutState s;                                                                  // (every lane, in front of the first barrier)
  {
    const double *sb = state + (size_t)b * 13;
    s.r0 = sb[0]; s.r1 = sb[1]; s.r2 = sb[2]; s.v0 = sb[3]; s.v1 = sb[4]; s.v2 = sb[5];
    s.qx = sb[6]; s.qy = sb[7]; s.qz = sb[8]; s.qw = sb[9]; s.w0 = sb[10]; s.w1 = sb[11]; s.w2 = sb[12];
  }
  const long long calls = count[b];
  int word = word_io[b];
  RolloutBody M;
  {
#pragma clang fp contract(off)
    const double ms = mass_scale ? mass_scale[b] : 1.0;
    M.m_s = A.mass * ms;
#pragma unroll
    for (int i = 0; i < 9; ++i) { M.I[i] = ms * A.Ib[i]; M.J[i] = A.Ii[i] / ms; }
    const double *pb = push ? push + (size_t)b * 6 : nullptr;
    M.F0 = pb ? pb[0] : 0.0; M.F1 = pb ? pb[1] : 0.0; M.F2 = pb ? pb[2] : 0.0;
    M.T0 = pb ? pb[3] : 0.0; M.T1 = pb ? pb[4] : 0.0; M.T2 = pb ? pb[5] : 0.0;
  }
  const RowSegment G = RowSegment::of(A.capacity, A.n_rows, A.first_row, n_rows, first_row, cursor, b);
  const long long rows_b = G.rows_b, n = G.n;
  if (n == 0) return;                                                              // (uniform: a window without rows keeps its state)
  const double *x = nodes + (size_t)b * S.n_vars;
  const double t0b = t0[b];
  double *meas_b = meas + (size_t)b * (size_t)rows_b * mcols;
  double *out_b = rows_out ? rows_out + (size_t)b * (size_t)rows_b * ROLLOUT_COLS : nullptr;
  double *feet_b = frows_out ? frows_out + (size_t)b * (size_t)rows_b * FEET_COLS : nullptr;
  double *qp_b = qrows_out ? qrows_out + (size_t)b * (size_t)rows_b * QP_COLS : nullptr;
  const double *joint_b = joint ? joint + (size_t)b * (size_t)rows_b * QTOS_CSV_COLS : nullptr;
  for (long long j0 = 0; j0 < n; j0 += TILE) {                                     // (n is uniform over the workgroup: so are the barriers)
    const int m = G.tile_rows(j0, TILE);
    const long long base = G.row(j0);
    if ((int)threadIdx.x < m) {                                                    // (A) a lane takes a row of the plan
      double row[QTOS_CSV_COLS];
      const double t = sample_row_state_at(S, x, t0b, G.plan_row(j0, threadIdx.x), A.hz, row);
      int mask = 0;
#pragma unroll
      for (int e = 0; e < NEE; ++e) {
        sample_spline(S.eef[e], x, t, 0, row + 25 + 3 * e);
        mask |= (Ft.stance[e][sample_segment(S.eem[e], t)] != 0 ? 1 : 0) << e;
      }
      double *dst = rollqp_tile + threadIdx.x * ROLLQP_PITCH;
      rollout_inputs(row, A.ff_scale, dst);
      feet_inputs(row, mask, Ft.w_min, dst);
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                                        // (B) the chain, in program order
#pragma clang fp contract(off)
      if (j0 == 0 && ((A.flags & 1) || (word & 32))) {                             // QTOS_ROLLOUT_INIT / _PENDING, as in k_rollout
        word &= ~32;
        const double *p = rollqp_tile;
        s.r0 = p[1]; s.r1 = p[2]; s.r2 = p[3]; s.v0 = p[4]; s.v1 = p[5]; s.v2 = p[6];
        s.qx = p[7]; s.qy = p[8]; s.qz = p[9]; s.qw = p[10];
        const double qx = s.qx, qy = s.qy, qz = s.qz, qw = s.qw;
        const double R0 = 1 - 2 * (qy * qy + qz * qz), R1 = 2 * (qx * qy - qz * qw), R2 = 2 * (qx * qz + qy * qw);
        const double R3 = 2 * (qx * qy + qz * qw), R4 = 1 - 2 * (qx * qx + qz * qz), R5 = 2 * (qy * qz - qx * qw);
        const double R6 = 2 * (qx * qz - qy * qw), R7 = 2 * (qy * qz + qx * qw), R8 = 1 - 2 * (qx * qx + qy * qy);
        s.w0 = (R0 * p[11] + R3 * p[12]) + R6 * p[13];
        s.w1 = (R1 * p[11] + R4 * p[12]) + R7 * p[13];
        s.w2 = (R2 * p[11] + R5 * p[12]) + R8 * p[13];
      }
      for (int i = 0; i < m; ++i) {
        double *p = rollqp_tile + i * ROLLQP_PITCH;
        double ex, ey, ez, ew;
        rollout_attitude(p, s, ex, ey, ez, ew);
        const double en = rollout_norm(s.r0 - p[1], s.r1 - p[2], s.r2 - p[3]);
        const double tilt = 2 * rollout_norm(ex, ey, ez);
        const bool finite = isfinite(s.r0) && isfinite(s.r1) && isfinite(s.r2) && isfinite(s.v0) && isfinite(s.v1) && isfinite(s.v2) &&
                            isfinite(s.qx) && isfinite(s.qy) && isfinite(s.qz) && isfinite(s.qw) && isfinite(s.w0) && isfinite(s.w1) &&
                            isfinite(s.w2);
        if (!finite) word |= 2;
        if ((A.dev_max > 0 && en > A.dev_max) || (A.tilt_max > 0 && tilt > A.tilt_max)) word |= 1;
        int st = word & 3;
        double *q = p + FEET_STATE;
        q[0] = s.r0; q[1] = s.r1; q[2] = s.r2; q[3] = s.v0; q[4] = s.v1; q[5] = s.v2;
        q[6] = s.qx; q[7] = s.qy; q[8] = s.qz; q[9] = s.qw; q[10] = s.w0; q[11] = s.w1; q[12] = s.w2;
        q[13] = en; q[14] = tilt;
        const int mask = (int)p[FEET_MASK];
        const int cnt = (mask & 1) + ((mask >> 1) & 1) + ((mask >> 2) & 1) + ((mask >> 3) & 1);
        int feet_bits = (cnt == 0 ? 64 : 0) | (cnt == 2 ? 128 : 0);
        double fbn = 0;
        if (!st) {
          const long long c = calls + j0 + i;
          const bool acts = push != nullptr && c >= A.push_from && c - A.push_from < A.push_ticks;
          bool clipped = false, limited = false;
          FeetOut first;
          FeetQp q1, q2;
          q1.Q = &Q; q1.slab = rollqp_slab; q2.Q = &Q; q2.slab = rollqp_slab;
          fbn = rollout_feet_step<true>(A, Ft, M, p, acts, s, clipped, limited, first, &q1);
          bool cap = q1.cap;
          for (int u = 1; u < A.substeps; ++u) {
            FeetOut later;
            rollout_feet_step<true>(A, Ft, M, p, acts, s, clipped, limited, later, &q2);
            cap = cap || q2.cap;
          }
#pragma unroll
          for (int k = 0; k < QP_COLS; ++k) p[ROLLQP_Q + k] = q1.col[k];           // (the solve's columns of the tick's first step)
          feet_bits |= cap ? 512 : 0;
#pragma unroll
          for (int k = 0; k < 12; ++k) p[FEET_F + k] = first.fa[k];               // (behind the tick's last step: it read f_e and w_e)
          p[FEET_W] = first.miss_f; p[FEET_W + 1] = first.miss_t; p[FEET_W + 2] = first.change;
          st = (clipped ? 8 : 0) | (acts ? 16 : 0) | (limited ? 256 : 0);
        } else {
          p[FEET_W] = 0.0; p[FEET_W + 1] = 0.0; p[FEET_W + 2] = 0.0;             // a frozen row: the plan's forces stay in their place
#pragma unroll
          for (int k = 0; k < QP_COLS; ++k) p[ROLLQP_Q + k] = 0.0;
        }
        q[15] = fbn; p[FEET_STATUS] = (double)(st | feet_bits);
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < m) {                                                    // (C) a lane turns its row's state into the output columns
      double *p = rollqp_tile + threadIdx.x * ROLLQP_PITCH;
      const int st = (int)p[FEET_STATUS] | rollout_output<FEET_STATE>(p);
      status_out[(size_t)b * (size_t)rows_b + G.tile_row(base, threadIdx.x)] = st;
    }
    __syncthreads();
    if (out_b) {                                                                   // the tile goes out flat: rows ...
      for (int e = threadIdx.x; e < m * ROLLOUT_COLS; e += TILE) {
        const int i = e / ROLLOUT_COLS, c = e - i * ROLLOUT_COLS;
        out_b[G.flat(base, ROLLOUT_COLS, e)] = rollqp_tile[i * ROLLQP_PITCH + c];
      }
    }
    if (feet_b) {                                                                  // ... the feet rows ...
      for (int e = threadIdx.x; e < m * FEET_COLS; e += TILE) {
        const int i = e / FEET_COLS, c = e - i * FEET_COLS;
        const double *p = rollqp_tile + i * ROLLQP_PITCH;
        feet_b[G.flat(base, FEET_COLS, e)] = c == 0 ? p[0] : (c < 13 ? p[FEET_F + (c - 1)] : p[FEET_W + (c - 13)]);
      }
    }
    if (qp_b) {                                                                    // ... the solve's columns ...
      for (int e = threadIdx.x; e < m * QP_COLS; e += TILE) {
        const int i = e / QP_COLS, c = e - i * QP_COLS;
        qp_b[G.flat(base, QP_COLS, e)] = rollqp_tile[i * ROLLQP_PITCH + ROLLQP_Q + c];
      }
    }
    for (int e = threadIdx.x; e < m * mcols; e += TILE) {                          // ... and meas
      const int i = e / mcols, c = e - i * mcols;
      const double *p = rollqp_tile + i * ROLLQP_PITCH;
      const long long o = G.flat(base, mcols, e);
      if (c < 3) meas_b[o] = p[1 + c];
      else if (c < mcols - 12) meas_b[o] = quat ? p[13 + (c - 3)] : p[4 + (c - 3)];
      else if (joint_b) meas_b[o] = joint_b[(size_t)G.tile_row(base, i) * QTOS_CSV_COLS + 1 + (c - (mcols - 12))];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double *sb = state + (size_t)b * 13;
    sb[0] = s.r0; sb[1] = s.r1; sb[2] = s.r2; sb[3] = s.v0; sb[4] = s.v1; sb[5] = s.v2;
    sb[6] = s.qx; sb[7] = s.qy; sb[8] = s.qz; sb[9] = s.qw; sb[10] = s.w0; sb[11] = s.w1; sb[12] = s.w2;
    count[b] = calls + n;
    word_io[b] = word;
  }
}

// Goals of receding windows from their global paths (qtos_path_goal*; Global_Planner.update / spine_step, QTOS/planner.py:139-161,
// 195-230; Combiner.plan_init / spine_step, QTOS/combiner.py:137-212): where the next plan goes.  One lane per window: the
// window's A* "spine" (two cubic splines in scipy's layout, global_planner.path_table) is read one horizon ahead of the new plan's
// start, the displacement from the base point is clipped to step_size per axis, and the goal height is the terrain under the
// goal + z_offset.  The statement of the rule is global_planner.path_goal, and this kernel equals it to the bit: every
// function below switches contraction off in its own body (the library is built with the compiler's default, which fuses
// a * b + c), so each operation is one rounded IEEE double operation, in scipy's order of summation, which is not Horner's.
// No LDS, no scratch: the tables come through pointers and are indexed per lane, the arguments hold scalars only (see
// k_handover), and no handle state is read or written.
struct PathGoalArgs {   // QtosPathGoal as the kernel reads it (window_api.hpp path_goal_args)
  double horizon, step_size, tol, z_offset, cell, origin_x, origin_y, t_stop, stop_dist;
  int base, clamp_x, advance_clock, hold_done;
  int n_paths, max_pieces, n_maps, rows, cols;
};

// One spine at time t (global_planner.spine_eval): x the path's n + 1 knots, c its coefficients c[k * mp + i] of (t - x[i])^(3 - k).
// The bisection counts the knots <= t, which is searchsorted(x[:n + 1], t, 'right'); a NaN counts none and gives a NaN.
__device__ inline double path_spine(const double *x, const double *c, int n, int mp, double t) {
#pragma clang fp contract(off)
  int lo = 0, hi = n + 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (x[mid] <= t) lo = mid + 1; else hi = mid;
  }
  const int i = lo - 1 < 0 ? 0 : (lo - 1 > n - 1 ? n - 1 : lo - 1);
  const double s = t - x[i];
  double res = 0.0, z = 1.0;
#pragma unroll
  for (int kp = 0; kp < 4; ++kp) {
    res = res + c[(size_t)(3 - kp) * mp + i] * z;
    z = z * s;
  }
  return res;
}

// GlobalPlanner.get_map_height (global_planner.map_height): the index test is made in double, so a huge or non-finite
// coordinate takes the fall-back cell and reads nothing else.  hm null: every height is 0.
__device__ inline double path_height(const PathGoalArgs &A, const double *hm, double x, double y) {
#pragma clang fp contract(off)
  if (!hm) return 0.0;
  const double fr = floor((y + A.origin_y) / A.cell), fc = floor((x + A.origin_x) / A.cell);
  int r = A.rows - 1, c = A.cols / 2;
  if (fr >= -(double)A.rows && fr < (double)A.rows && fc >= -(double)A.cols && fc < (double)A.cols) {
    r = (int)fr; c = (int)fc;
    if (r < 0) r += A.rows;        // (Python's wrap of a negative index)
    if (c < 0) c += A.cols;
  }
  return hm[(size_t)r * A.cols + c];
}

__device__ inline double path_clip(double d, double step) {   // np.clip(d, -step, step), step >= 0: a NaN stays a NaN
  return d < -step ? -step : (d > step ? step : d);
}

__global__ __launch_bounds__(64) void k_path_goal(PathGoalArgs A, const double *knots, const double *coef, const int *n_pieces,
                                                  const double *robot_goal, const int *path_id, const double *height_yx,
                                                  const int *map_id, double *clock, const double *offset, const double *start,
                                                  double *goal_out, int *done, int B) {
#pragma clang fp contract(off)
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  int p = path_id ? path_id[b] : b;
  p = p < 0 ? 0 : (p > A.n_paths - 1 ? A.n_paths - 1 : p);       // (an id outside the table reads its nearest path, never beyond it)
  int n = n_pieces[p];
  n = n < 1 ? 1 : (n > A.max_pieces ? A.max_pieces : n);
  const double *x = knots + (size_t)p * (A.max_pieces + 1);
  const double *cx = coef + (size_t)p * 8 * A.max_pieces, *cy = cx + (size_t)4 * A.max_pieces;
  const double *hm = nullptr;
  if (height_yx) {
    int m = map_id ? map_id[b] : 0;
    m = m < 0 ? 0 : (m > A.n_maps - 1 ? A.n_maps - 1 : m);
    hm = height_yx + (size_t)m * A.rows * A.cols;
  }
  const double *st = start ? start + (size_t)b * QTOS_START_DOUBLES : nullptr;
  const double lt = clock[b] + (offset ? offset[b] : 0.0);       // plan time of the new plan's row 0
  const double tf = lt + A.horizon;
  double sx = path_spine(x, cx, n, A.max_pieces, tf), sy = path_spine(x, cy, n, A.max_pieces, tf);
  if (!(fabs(sx) > A.tol)) sx = 0.0;
  if (!(fabs(sy) > A.tol)) sy = 0.0;
  const double gz = path_height(A, hm, sx, sy) + A.z_offset;
  if (A.clamp_x) {                                               // Combiner.spine_step: behind the height, as the reference does
    const double rgx = robot_goal[(size_t)p * 3];
    if (sx > rgx) sx = rgx;
  }
  double bx, by, bz;
  if (A.base == 0) {                                             // Global_Planner.update: the spine at the plan's start
    bx = path_spine(x, cx, n, A.max_pieces, lt);
    by = path_spine(x, cy, n, A.max_pieces, lt);
    bz = path_height(A, hm, bx, by) + A.z_offset;
  } else {                                                       // plan_init, spine_step(com, t): the state the plan starts from
    bx = st[0]; by = st[1]; bz = st[2];
  }
  double gx = bx + path_clip(sx - bx, A.step_size), gy = by + path_clip(sy - by, A.step_size);
  double gzc = bz + path_clip(gz - bz, A.step_size);
  int bits = 0;
  if (x[n] < lt - A.t_stop) bits |= 1;                           // the path's end lies t_stop behind the plan's start
  if (A.stop_dist > 0) {
    const double dx = st[0] - gx, dy = st[1] - gy;
    if (sqrt(dx * dx + dy * dy) < A.stop_dist) bits |= 2;
  }
  int d = 0;
  if (done) {
    d = done[b] | bits;
    done[b] = d;
  }
  if (A.hold_done && d) { gx = st[0]; gy = st[1]; gzc = st[2]; }  // a finished window stands still
  goal_out[(size_t)b * 3 + 0] = gx;
  goal_out[(size_t)b * 3 + 1] = gy;
  goal_out[(size_t)b * 3 + 2] = gzc;
  if (A.advance_clock) clock[b] = lt;
}

// The global paths of receding windows (qtos_path_plan*; PATH_Solver, QTOS/planner.py:282-457): what k_path_goal reads, made on
// the device.  One wavefront per window: A* over the window's boolean map, every second cell of the path a point of two
// not-a-knot cubics.  The statement of the rule is global_planner.path_plan (path_cells, spine_fit), and this kernel equals it to
// the bit: the cells because every pop is an exact lexicographic minimum of (f, cell), the numbers because every function
// below switches contraction off and performs the rule's operations one by one.
// LDS, laid out for the limits the host checks (rows * cols <= PP_GRID, max_open <= PP_OPEN, max_cells <= PP_GRID), PP_LDS_BYTES
// (139264) in all:
//   cw   PP_GRID x u32   per cell: bits 0-16 g (an integer: every step costs 1.0; at most the number of pops, 4 * PP_GRID + 4),
//                        17-18 the direction it was reached by, 19 closed, 20 blocked
//   live PP_GRID x u16   per cell: its entries in the open list (<= max_open); after the search the path's cells
//   of   PP_OPEN x f64   the open list's f, unsorted          oc   PP_OPEN x u16   and cells (row * cols + col)
// The search is uniform over the wave: every lane follows it, the lanes share the pop (a strided scan and six butterfly
// steps) and lane 0 stores.  No scratch, plain vector stores only, no handle state.
constexpr int PP_GRID = 16384, PP_OPEN = 4096;
constexpr int PP_LDS_BYTES = PP_GRID * 4 + PP_GRID * 2 + PP_OPEN * 8 + PP_OPEN * 2;
constexpr unsigned PP_G = 0x1ffffu, PP_CLOSED = 1u << 19, PP_BLOCKED = 1u << 20;
struct PathPlanArgs {   // QtosPathPlan as the kernel reads it (window_api.hpp path_plan_args)
  double cell, origin_x, origin_y, height_bound, step_size;
  int rows, cols, max_cells, max_open, max_pieces, n_maps, set_done;
};

// floor((v + o) / cell) as an int32 cell index; false where it is not finite or does not fit
__device__ inline bool pp_cell_of(double v, double o, double cell, int *out) {
#pragma clang fp contract(off)
  const double f = floor((v + o) / cell);
  if (!(f >= -2147483648.0 && f <= 2147483647.0)) return false;
  *out = (int)f;
  return true;
}

// (f, cell, slot) < (f2, cell2, slot2): f as the bits of a double >= 0, which order as the doubles do; the slot only makes the
// order total, so that every lane of the butterfly ends on the same entry
__device__ inline void pp_take_less(unsigned long long &f, int &c, int &k, unsigned long long f2, int c2, int k2) {
  if (f2 < f || (f2 == f && (c2 < c || (c2 == c && k2 < k)))) { f = f2; c = c2; k = k2; }
}

// The path's point i of n + 1 on one axis (0: x from the columns, 1: y from the rows): cell * cell_size - origin over every
// second cell, the last cell WITHOUT the shift (sic, QTOS/planner.py:410,412).  The start cell is not in the LDS list.
__device__ inline double pp_point(const unsigned short *path, int n_cells, int n, int cols, int sr, int sc, int axis, double cell,
                                  double origin, int i) {
#pragma clang fp contract(off)
  const int j = i < n ? 2 * i : n_cells - 1;
  int r = sr, c = sc;
  if (j > 0) { r = path[j] / cols; c = path[j] % cols; }
  const double v = (double)(axis ? r : c) * cell;
  return i < n ? v - origin : v;
}

__device__ inline double pp_knot(double T, int n, int i) {   // numpy's linspace(0, T, n + 1)
#pragma clang fp contract(off)
  return i >= n ? T : (double)i * (T / (double)n);
}

// global_planner.spine_fit for one axis, by one lane: c = the window's 4 x mp coefficient rows, which are also the work space
// (c' in row 0, g' and then s from row 2 on: s[i] is already c2[i], and the last pass runs downwards so that c3 never
// overwrites the s[n] that spills into row 3 where n = mp).
__device__ inline void pp_spine_fit(double *c, int mp, const unsigned short *path, int n_cells, int n, int cols, int sr, int sc, int axis,
                                    double cell, double origin, double T) {
#pragma clang fp contract(off)
  auto Y = [&](int i) { return pp_point(path, n_cells, n, cols, sr, sc, axis, cell, origin, i); };
  auto H = [&](int i) { return pp_knot(T, n, i + 1) - pp_knot(T, n, i); };
  auto D = [&](int i) { return (Y(i + 1) - Y(i)) / H(i); };
  double *s = c + (size_t)2 * mp;
  if (n == 1) {
    const double d0 = D(0);
    s[0] = d0; s[1] = d0;
  } else if (n == 2) {
    const double h0 = H(0), h1 = H(1), d0 = D(0), d1 = D(1);
    const double b0 = 2.0 * d0, b1 = 3.0 * (h0 * d1 + h1 * d0), b2 = 2.0 * d1;
    const double s1 = ((b1 - h1 * b0) - h0 * b2) / ((2.0 * (h0 + h1) - h1) - h0);
    s[0] = b0 - s1; s[1] = s1; s[2] = b2 - s1;
  } else {
    double hp = H(0), dp = D(0), hi = H(1), di = D(1);            // h, d of rows i - 1 and i
    double dd = pp_knot(T, n, 2) - pp_knot(T, n, 0);
    double b = ((hp + 2.0 * dd) * hi * dp + hp * hp * di) / dd;
    double cp = dd / hi, gp = b / hi;
    c[0] = cp; s[0] = gp;
    for (int i = 1; i < n; ++i) {
      if (i > 1) { hp = hi; dp = di; hi = H(i); di = D(i); }
      b = 3.0 * (hi * dp + hp * di);
      const double den = 2.0 * (hp + hi) - hi * cp;
      cp = hp / den;
      gp = (b - hi * gp) / den;
      c[i] = cp; s[i] = gp;
    }
    // (hp, dp, hi, di are now those of rows n - 2 and n - 1)
    dd = pp_knot(T, n, n) - pp_knot(T, n, n - 2);
    b = (hi * hi * dp + (2.0 * dd + hi) * hp * di) / dd;
    const double den = hp - dd * cp;
    double sn = (b - dd * gp) / den;
    s[n] = sn;
    for (int i = n - 1; i >= 0; --i) {
      sn = s[i] - c[i] * sn;
      s[i] = sn;
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    const double h = H(i), d = D(i), si = s[i], t = ((si + s[i + 1]) - 2.0 * d) / h;
    c[i] = t / h;
    c[(size_t)mp + i] = (d - si) / h - t;
    c[(size_t)3 * mp + i] = Y(i);                                  // (c2[i] = s[i] stands where it is)
  }
}

__global__ __launch_bounds__(64) void k_path_plan(PathPlanArgs A, const double *bool_maps, const int *map_id, const double *start,
                                                  const double *robot_goal, double *knots, double *coef, int *n_pieces, int *cells,
                                                  int *n_cells_out, int *status_out, int *done) {
#pragma clang fp contract(off)
  __shared__ unsigned cw[PP_GRID];
  __shared__ unsigned short live[PP_GRID];
  __shared__ double of[PP_OPEN];
  __shared__ unsigned short oc[PP_OPEN];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int rows = A.rows, cols = A.cols, N = rows * cols, mp = A.max_pieces;
  const double x0 = start[(size_t)b * QTOS_START_DOUBLES], y0 = start[(size_t)b * QTOS_START_DOUBLES + 1];
  const double gx = robot_goal[(size_t)b * 3], gy = robot_goal[(size_t)b * 3 + 1];
  int m = map_id ? map_id[b] : 0;
  m = m < 0 ? 0 : (m > A.n_maps - 1 ? A.n_maps - 1 : m);           // (an id outside reads its nearest map, never beyond them)
  const double *bm = bool_maps + (size_t)m * N;
  for (int i = lane; i < N; i += 64) {
    cw[i] = bm[i] > A.height_bound ? PP_BLOCKED : 0u;
    live[i] = 0;
  }
  __syncthreads();

  int sr = 0, sc = 0, gr = 0, gc = 0;
  int status = 0, n_cells = 0;
  if (!pp_cell_of(y0, A.origin_y, A.cell, &sr) || !pp_cell_of(x0, A.origin_x, A.cell, &sc) || !pp_cell_of(gy, A.origin_y, A.cell, &gr) ||
      !pp_cell_of(gx, A.origin_x, A.cell, &gc))
    status = 1;
  if (status == 0) {
    // ---- PathSolver.astar ----
    int n_open = 0, pops = 0;
    long long r = sr, c = sc;                                      // (the start may lie anywhere in the int32 range: its neighbours in 64 bits)
    bool found = false;
    while (true) {
      if (pops > 0) {                                              // (the first pop is the start: the list's only entry)
        if (n_open == 0) { status = 1; break; }
        unsigned long long bf = ~0ull;
        int bc = 0x7fffffff, bk = 0x7fffffff;
        for (int k = lane; k < n_open; k += 64) pp_take_less(bf, bc, bk, (unsigned long long)__double_as_longlong(of[k]), (int)oc[k], k);
        for (int off = 32; off; off >>= 1) {
          const unsigned long long f2 = __shfl_xor(bf, off);
          const int c2 = __shfl_xor(bc, off), k2 = __shfl_xor(bk, off);
          pp_take_less(bf, bc, bk, f2, c2, k2);
        }
        const int k = __builtin_amdgcn_readfirstlane(bk), ci = __builtin_amdgcn_readfirstlane(bc);
        --n_open;
        if (lane == 0) {                                           // swap with the last
          of[k] = of[n_open];
          oc[k] = oc[n_open];
          live[ci] = live[ci] - 1;
        }
        __syncthreads();
        r = ci / cols; c = ci % cols;
      }
      if (++pops > 4 * N + 4) { status = 3; break; }
      if (r == gr && c == gc) { found = true; break; }
      int gcur = 0;
      if (r >= 0 && r < rows && c >= 0 && c < cols) {
        const int ci = (int)r * cols + (int)c;
        gcur = (int)(cw[ci] & PP_G);
        if (lane == 0) cw[ci] = cw[ci] | PP_CLOSED;
      }
      for (int d = 0; d < 4; ++d) {                                // (0, 1), (0, -1), (1, 0), (-1, 0)
        const long long nr = r + (d == 2 ? 1 : (d == 3 ? -1 : 0)), nc = c + (d == 0 ? 1 : (d == 1 ? -1 : 0));
        if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) continue;
        const int ni = (int)nr * cols + (int)nc;
        const unsigned w = cw[ni];
        if (w & PP_BLOCKED) continue;
        const int gn = gcur + 1, gnb = (int)(w & PP_G);
        if ((w & PP_CLOSED) && gn >= gnb) continue;
        if (gn < gnb || live[ni] == 0) {
          if (n_open >= A.max_open) { status = 3; break; }
          const double dr = (double)((long long)gr - nr), dc = (double)((long long)gc - nc);
          const double f = (double)gn + sqrt(dr * dr + dc * dc);
          if (lane == 0) {
            cw[ni] = (w & PP_CLOSED) | ((unsigned)d << 17) | (unsigned)gn;
            of[n_open] = f;
            oc[n_open] = (unsigned short)ni;
            live[ni] = live[ni] + 1;
          }
          ++n_open;
        }
      }
      __syncthreads();
      if (status) break;
    }
    if (found) {
      // ``while current in came_from``: inside the grid and reached by a step (g > 0); the start never is
      int len = 0;
      long long wr = r, wc = c;
      while (wr >= 0 && wr < rows && wc >= 0 && wc < cols && len <= N) {
        const unsigned w = cw[(int)wr * cols + (int)wc];
        if ((w & PP_G) == 0) break;
        const int d = (int)((w >> 17) & 3u);
        wr -= (d == 2 ? 1 : (d == 3 ? -1 : 0));
        wc -= (d == 0 ? 1 : (d == 1 ? -1 : 0));
        ++len;
      }
      n_cells = len + 1;
      if (n_cells > A.max_cells) status = 2;
      else if (lane == 0) {                                        // the path's cells behind the start, in `live`
        wr = r; wc = c;
        for (int j = len; j >= 1; --j) {
          const int ci = (int)wr * cols + (int)wc;
          live[j] = (unsigned short)ci;
          const int d = (int)((cw[ci] >> 17) & 3u);
          wr -= (d == 2 ? 1 : (d == 3 ? -1 : 0));
          wc -= (d == 0 ? 1 : (d == 1 ? -1 : 0));
        }
      }
    }
  }
  __syncthreads();
  if (status != 0 && status != 2) n_cells = 0;

  const double dx = x0 - gx, dy = y0 - gy;
  const double T = sqrt(dx * dx + dy * dy) / A.step_size * 10.0;
  if (status == 0 && !(T > 0)) status = 4;
  const int n = status == 0 ? (n_cells + 1) / 2 : 1;               // sub = path[::2]
  double *kn = knots + (size_t)b * (mp + 1), *cf = coef + (size_t)b * 8 * mp;
  if (cells) {
    int *cl = cells + (size_t)b * A.max_cells * 2;
    for (int j = lane; j < A.max_cells; j += 64) {
      int pr = 0, pc = 0;
      if (status == 0 || status == 4) {
        if (j == 0) { pr = sr; pc = sc; }
        else if (j < n_cells) { pr = live[j] / cols; pc = live[j] % cols; }
      }
      cl[2 * j] = pr;
      cl[2 * j + 1] = pc;
    }
  }
  for (int i = lane; i <= mp; i += 64) kn[i] = status == 0 ? pp_knot(T, n, i) : 0.0;
  if (status == 0) {
    if (lane < 2)
      pp_spine_fit(cf + (size_t)lane * 4 * mp, mp, live, n_cells, n, cols, sr, sc, lane, A.cell, lane ? A.origin_y : A.origin_x, T);
  } else if (lane < 2) {
    cf[(size_t)lane * 4 * mp + (size_t)3 * mp] = lane ? y0 : x0;   // the constant spine at the start point
  }
  __syncthreads();                                                 // (the fit's work space lies in the padding where n < mp)
  for (int i = lane; i < 8 * mp; i += 64) {
    const int col = i % mp, row = (i / mp) & 3;
    if (col >= n || (status != 0 && row != 3)) cf[i] = 0.0;
  }
  if (lane == 0) {
    n_pieces[b] = n;
    n_cells_out[b] = n_cells;
    status_out[b] = status;
    if (done && A.set_done && status != 0) done[b] = done[b] | 4;
  }
}

// The probe and the stamp of the windows' heightfields (qtos_probe*, qtos_probe_stamp*; PATH_MAP.probe_map and worker_f,
// QTOS/generateHeightField.py:172-404): what k_path_plan reads as bool_maps, made on the device with the batched solve between
// the two steps.  The statement of the rule is feasibility.probe_table / round2 / stamp_table, and these kernels equal it to
// the bit: every function that forms a coordinate switches contraction off and performs the rule's operations one by one (the
// one explicit fma of probe_round2 is the exact error of a product).  One wavefront per map.  The placement of the patches is
// decided by counting alone: k_probe_count leaves every map's number of patches in offsets[m + 1], k_probe_scan turns them into
// prefix sums in place, and k_probe places patch q of map m at offsets[m] + (the candidates in front of q in queue order), a
// ballot and a prefix count per 64 candidates.  No atomics, no scratch, plain vector stores only, no handle state.
// LDS (k_probe), dynamic, sized at the launch by probe_lds_bytes: the map's row coordinates, its column coordinates and the
// twelve stance offsets, rows + cols / 2 + 12 doubles (a 20 x 60 map: 496 B; with rows * cols <= 16384 at most 64 KiB).
struct ProbeArgs {   // QtosProbe as the kernels read it (window_api.hpp probe_args)
  double cell, origin_shift, z_offset, stance[QTOS_NEE * 3];
  int rows, cols, n_maps, scale, multi_map_shift, capacity;
};

inline size_t probe_lds_bytes(int rows, int cols) { return ((size_t)rows + (size_t)(cols / 2) + QTOS_NEE * 3) * sizeof(double); }

// Python's round(v, 2) (feasibility.round2): the product's exact error decides the half-way cases that are no true ties
__device__ inline double probe_round2(double v) {
#pragma clang fp contract(off)
  const double p = v * 100.0;
  const double e = fma(v, 100.0, -p);
  double k = rint(p);
  if (fabs(p - k) == 0.5 && e != 0.0) k = floor(p) + (e > 0.0 ? 1.0 : 0.0);
  return k / 100.0;
}

// neighbors_danger_test(m, r, c): the eight neighbours in the reference's order; the first one outside the map answers false,
// the first one inside it that is > 0 answers true (a NaN is not > 0)
__device__ inline bool probe_danger(const double *hm, int rows, int cols, int r, int c) {
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int nr = r + ((k == 0 || k == 4 || k == 5) ? 1 : ((k == 1 || k == 6 || k == 7) ? -1 : 0));
    const int nc = c + ((k == 2 || k == 4 || k == 7) ? 1 : ((k == 3 || k == 5 || k == 6) ? -1 : 0));
    if (nr < 0 || nr >= rows || nc < 0 || nc >= cols) return false;
    if (hm[(size_t)nr * cols + nc] > 0.0) return true;
  }
  return false;
}

// candidate q = row * nj + j of a map (queue order): the patch from column 2 j to column 2 j + 2 of that row
__device__ inline bool probe_candidate(const double *hm, int rows, int cols, int nj, int q) {
  const int r = q / nj, c = 2 * (q % nj);
  return probe_danger(hm, rows, cols, r, c) || probe_danger(hm, rows, cols, r, c + 2);
}

__global__ __launch_bounds__(64) void k_probe_count(ProbeArgs A, const double *map_yx, int *offsets) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int rows = A.rows, cols = A.cols, nj = cols / 2 - 1, Q = rows * nj;
  const double *hm = map_yx + (size_t)m * rows * cols;
  int n = 0;
  for (int q0 = 0; q0 < Q; q0 += 64) {
    const int q = q0 + lane;
    const bool cand = q < Q && probe_candidate(hm, rows, cols, nj, q);
    n += __popcll(__ballot(cand));
  }
  if (lane == 0) {
    offsets[m + 1] = n;
    if (m == 0) offsets[0] = 0;
  }
}

// offsets[1 .. n_maps]: counts -> inclusive prefix sums, in place, by one workgroup (a lane owns a contiguous run of entries)
__global__ __launch_bounds__(256) void k_probe_scan(int *offsets, int n_maps) {
  __shared__ int part[256];
  const int t = threadIdx.x, per = (n_maps + 255) / 256;
  const int lo = 1 + t * per, hi = lo + per < n_maps + 1 ? lo + per : n_maps + 1;
  int s = 0;
  for (int i = lo; i < hi; ++i) s += offsets[i];
  part[t] = s;
  __syncthreads();
  int run = 0;
  for (int k = 0; k < t; ++k) run += part[k];
  for (int i = lo; i < hi; ++i) {
    run += offsets[i];
    offsets[i] = run;
  }
}

__global__ __launch_bounds__(64) void k_probe(ProbeArgs A, const double *map_yx, const int *offsets, int *slot, int *patch, double *start,
                                              double *goal, int *map_id) {
#pragma clang fp contract(off)
  extern __shared__ double co[];                                     // ys[rows], xs[nj + 1] (xs[j] starts patch j, xs[j + 1] is its goal), stance[12]
  const int m = blockIdx.x, lane = threadIdx.x;
  const int rows = A.rows, cols = A.cols, nj = cols / 2 - 1, Q = rows * nj;
  if (Q < 1) return;                                                 // (uniform: a map of 2 or 3 columns has no candidate and no slot)
  const double *hm = map_yx + (size_t)m * rows * cols;
  double *ys = co, *xs = co + rows, *stance = xs + nj + 1;           // (the stance is read per patch: in LDS it holds no scalar registers over the loop)
  if (lane == 0) {                                                   // PATH_MAP.probe_map's walk, statement by statement
#pragma unroll
    for (int k = 0; k < QTOS_NEE * 3; ++k) stance[k] = A.stance[k];
    const double res = A.cell * (1.0 / (double)A.scale), half = (double)cols / 2.0;
    const double shift = (double)(A.multi_map_shift - 1) * A.origin_shift;
    const double x_start = ((-res * half) - res / 2.0) + shift;      // (sic: x and y both start from the number of columns)
    const double x_goal = ((-res * half) + res / 2.0) + shift;
    double y = x_start;
    for (int r = 0; r < rows; ++r) {
      y = probe_round2(y + res);
      ys[r] = y;
    }
    xs[0] = probe_round2(x_start + res);
    double xg = x_goal;
    for (int j = 0; j < nj; ++j) {
      xg = probe_round2(xg + 2.0 * res);
      xs[j + 1] = xg;
    }
  }
  __syncthreads();
  int run = offsets[m];
  for (int q0 = 0; q0 < Q; q0 += 64) {
    const int q = q0 + lane;
    const bool cand = q < Q && probe_candidate(hm, rows, cols, nj, q);
    const unsigned long long mask = __ballot(cand);
    const int i = run + __popcll(mask & ((1ull << lane) - 1ull));
    run += __popcll(mask);
    if (q < Q) slot[(size_t)m * Q + q] = cand ? i : -1;
    if (!cand || i >= A.capacity) continue;                          // (nothing is written beyond the capacity)
    const int r = q / nj, j = q % nj;
    const double px = xs[j], py = ys[r], z = hm[(size_t)r * cols + 2 * j], zg = hm[(size_t)r * cols + 2 * j + 2];
    patch[(size_t)i * 3] = m;
    patch[(size_t)i * 3 + 1] = r;
    patch[(size_t)i * 3 + 2] = 2 * j;
    if (map_id) map_id[i] = m;
    if (start) {
      double *s = start + (size_t)i * QTOS_START_DOUBLES;
      s[0] = px; s[1] = py; s[2] = z + A.z_offset;
      s[3] = 0.0; s[4] = 0.0; s[5] = 0.0;
#pragma unroll
      for (int e = 0; e < QTOS_NEE; ++e) {
        s[6 + 3 * e] = stance[3 * e] + px;
        s[7 + 3 * e] = stance[3 * e + 1] + py;
        s[8 + 3 * e] = stance[3 * e + 2] + z;
      }
#pragma unroll
      for (int k = 18; k < QTOS_START_DOUBLES; ++k) s[k] = 0.0;
    }
    if (goal) {
      goal[(size_t)i * 3] = xs[j + 1];
      goal[(size_t)i * 3 + 1] = py;
      goal[(size_t)i * 3 + 2] = zg + A.z_offset;
    }
  }
}

// worker_f's stamp (feasibility.stamp_table): one lane per cell in turn.  The cell holds what the LAST patch of its map in queue
// order that writes it leaves, and that patch is the largest (row, j) among the few whose start or goal lies within the
// diamond's radius R = 3 scale of the cell (a failure), or on the cell and up to two cells left of it (a success: start, the
// cell right of it, goal).  The rows are walked downwards from r + R, the patches of a row downwards from the last whose
// diamonds reach the cell; the first patch met that writes the cell decides.  A slot beyond offsets[n_maps] is no patch.
__global__ __launch_bounds__(64) void k_probe_stamp(ProbeArgs A, const int *offsets, const int *slot, const int *status, double *bool_maps) {
  const int m = blockIdx.x, lane = threadIdx.x;
  const int rows = A.rows, cols = A.cols, nj = cols / 2 - 1, R = 3 * A.scale, N = offsets[A.n_maps];
  const int *sl = slot + (size_t)m * rows * (nj > 0 ? nj : 0);
  double *bm = bool_maps + (size_t)m * rows * cols;
  for (int ci = lane; ci < rows * cols; ci += 64) {
    const int r = ci / cols, c = ci % cols;
    double v = 0.0;
    bool found = false;
    const int r_hi = r + R < rows - 1 ? r + R : rows - 1, r_lo = r - R > 0 ? r - R : 0;
    for (int pr = r_hi; pr >= r_lo && !found; --pr) {
      const int w = R - (pr > r ? pr - r : r - pr);                  // the diamond's reach along this row (>= 0)
      int j_hi = (c + w) >> 1, j_lo = (c - w - 2 + 1) >> 1;          // start columns 2 j within c - w - 2 .. c + w
      if (j_hi > nj - 1) j_hi = nj - 1;
      if (j_lo < 0) j_lo = 0;
      for (int j = j_hi; j >= j_lo; --j) {
        const int i = sl[(size_t)pr * nj + j];
        if (i < 0 || i >= N) continue;
        const int st = status[i], d = c - 2 * j, ds = d < 0 ? -d : d, dg = d < 2 ? 2 - d : d - 2;   // columns from the start, the goal
        if (st != 0 ? (ds <= w || dg <= w) : (pr == r && d >= 0 && d <= 2)) {
          v = st != 0 ? 1.0 : 0.0;
          found = true;
          break;
        }
      }
    }
    bm[ci] = v;
  }
}

// The randomised terrain of the windows (qtos_terrain_env*; Height_Map_Generator.__init__ with randomize_env and update(),
// QTOS/generateHeightField.py:563-567, 584-588, 648-730): what qtos_set_heightfields_device, k_probe and k_path_goal read, made
// on the device from base grids and one seed per map.  The statement of the rule is heightfield.random_env_table, and this
// kernel equals it to the bit.  One workgroup of ENV_T lanes per map.  The stream is python's: MT19937 in LDS, seeded by one
// lane as random.seed(int) seeds it, regenerated by all lanes (a lane owns word t of each of the three runs [0, 227),
// [227, 454), [454, 623) whose words depend on the run in front alone, so it needs its own results only; word 623 follows).
// Every lane reads the same words and draws the same numbers, so the control flow is uniform and the barriers of a
// regeneration are met by all.  A level is a distinct value != 0 of the grid; the levels come out ascending from repeated
// min-reductions over the grid, lane j of every wave then keeps level j in a register, and the height passes run on those
// registers -- the solver copy's passes for their draws alone -- with a wave-wide min per snapshot entry.  The grid is touched
// again only to be written: each cell finds its level's slot by bisection and takes the slot's value, rolled by the net shift,
// in both orientations.  No atomics, no scratch, plain vector stores.
constexpr int ENV_T = 256;
struct TerrainEnvArgs {   // QtosTerrainEnv as the kernel reads it (window_api.hpp terrain_env_args)
  double delta;
  int n_maps, n_base, rows, cols, n_shift, n_height, climb;
};
struct EnvLds {
  unsigned mt[624];
  double level[QTOS_ENV_MAX_LEVELS];   // the base grid's levels, ascending: a cell's slot is the index of its value here
  double value[QTOS_ENV_MAX_LEVELS];   // what the slots hold behind the map's height passes
  double red[ENV_T / 64];              // a block-wide reduction's partial minima, and whether a wave found a candidate
  int found[ENV_T / 64];
};
static_assert(sizeof(EnvLds) == QTOS_ENV_LDS_BYTES, "QTOS_ENV_LDS_BYTES (qtos_planner.h) is k_terrain_env's LDS");

__device__ inline unsigned env_mix(unsigned a, unsigned b) {
  const unsigned y = (a & 0x80000000u) | (b & 0x7fffffffu);
  return (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
}

// the next 624 words of the state; called by all lanes of the workgroup
__device__ inline void env_twist(unsigned *mt, int tid) {
  unsigned n1 = 0, n2 = 0, n3 = 0;
  const unsigned last = mt[623];
  if (tid < 227) {
    n1 = mt[tid + 397] ^ env_mix(mt[tid], mt[tid + 1]);
    n2 = n1 ^ env_mix(mt[tid + 227], mt[tid + 228]);
    if (tid < 169) n3 = n2 ^ env_mix(mt[tid + 454], mt[tid + 455]);
  }
  __syncthreads();                     // the old state has been read, by this regeneration and by every wave's draws
  if (tid < 227) {
    mt[tid] = n1;
    mt[tid + 227] = n2;
    if (tid < 169) mt[tid + 454] = n3;
  }
  __syncthreads();
  if (tid == 0) mt[623] = mt[396] ^ env_mix(last, mt[0]);
  __syncthreads();
}

// random.seed(s) for 0 <= s < 2^64 (init_by_array on the seed's 32-bit words, low word first); one lane
__device__ inline void env_seed(unsigned *mt, unsigned long long s) {
  const unsigned key[2] = {(unsigned)s, (unsigned)(s >> 32)};
  const int nk = key[1] ? 2 : 1;
  unsigned prev = 19650218u;
  mt[0] = prev;
  for (int i = 1; i < 624; ++i) {
    prev = 1812433253u * (prev ^ (prev >> 30)) + (unsigned)i;
    mt[i] = prev;
  }
  int i = 1, j = 0;
  prev = mt[0];
  for (int k = 0; k < 624; ++k) {
    prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1664525u)) + (j ? key[1] : key[0]) + (unsigned)j;
    mt[i] = prev;
    j = j + 1 < nk ? j + 1 : 0;
    if (++i >= 624) { mt[0] = prev; i = 1; }
  }
  for (int k = 0; k < 623; ++k) {
    prev = (mt[i] ^ ((prev ^ (prev >> 30)) * 1566083941u)) - (unsigned)i;
    mt[i] = prev;
    if (++i >= 624) { mt[0] = prev; i = 1; }
  }
  mt[0] = 0x80000000u;
}

struct EnvStream {   // a lane's view of the workgroup's stream: the same in every lane
  unsigned *mt;
  int tid, pos, used;
  __device__ inline unsigned bits32() {
    if (pos >= 624) {
      env_twist(mt, tid);
      pos = 0;
    }
    unsigned y = __builtin_amdgcn_readfirstlane(mt[pos]);
    ++pos; ++used;
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    return y ^ (y >> 18);
  }
  __device__ inline void skip(int n) {                     // whole states are passed over without tempering them
    while (n > 0) {
      if (pos >= 624) {
        env_twist(mt, tid);
        pos = 0;
      }
      const int step = n < 624 - pos ? n : 624 - pos;
      pos += step;
      n -= step;
    }
  }
  __device__ inline int below(int n, int k) {              // choice among n items, k = bit_length(n)
    unsigned r = bits32() >> (32 - k);
    while (r >= (unsigned)n) r = bits32() >> (32 - k);
    return (int)r;
  }
  __device__ inline double uniform(double a, double w) {   // a + (b - a) * random(), w = b - a: the product and the sum round apart
#pragma clang fp contract(off)
    const unsigned hi = bits32() >> 5, lo = bits32() >> 6;
    const double r = ((double)hi * 67108864.0 + (double)lo) / 9007199254740992.0;
    const double p = w * r;
    return a + p;
  }
};

__device__ inline double env_wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// one pass of random_height over the level values a wave keeps one per lane (v; 0 in the lanes behind the last level)
__device__ inline void env_level_pass(EnvStream &S, double &v, int lane, double a, double w) {
#pragma clang fp contract(off)
  double snap = 0.0, last = 0.0;
  int n = 0;
  for (;;) {                                               // the snapshot: entry j, ascending, into lane j
    const bool cand = v != 0.0 && (n == 0 || v > last);
    if (!__ballot(cand)) break;
    last = env_wave_min(cand ? v : __builtin_huge_val());
    if (lane == n) snap = last;
    ++n;
  }
  for (int j = 0; j < n; ++j) {
    const double h = __shfl(snap, j);
    const double d = S.uniform(a, w);
    const int c = S.below(3, 2);
    if (v == h) {
      if (c == 0) v += d;
      else if (c == 1) v -= d;
    }
  }
}

__global__ __launch_bounds__(ENV_T) void k_terrain_env(TerrainEnvArgs A, const double *base_yx, const int *base_id,
                                                       const unsigned long long *seed, int *draws, double *map_yx, double *height_xy,
                                                       int *status) {
#pragma clang fp contract(off)
  __shared__ EnvLds L;
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int rows = A.rows, cols = A.cols, cells = rows * cols;
  const int skip = draws ? draws[m] : 0;
  if (skip < 0 || skip > QTOS_ENV_MAX_DRAWS) {             // (uniform: every lane read the same word)
    if (tid == 0) status[m] = 2;
    return;
  }
  const int b = base_id ? base_id[m] : m;
  if (b < 0 || b >= A.n_base) {                            // (uniform; never outside the base grids, whatever base_id holds)
    if (tid == 0) status[m] = 4;
    return;
  }
  const double *g = base_yx + (size_t)b * cells;

  // the levels, ascending: a min-reduction over the grid per level; the first one also looks for a NaN
  int n_levels = 0;
  double last = 0.0;
  for (;;) {
    double best = __builtin_huge_val();
    bool cand = false, nan = false;
    for (int ci = tid; ci < cells; ci += ENV_T) {
      const double v = g[ci];
      nan = nan || v != v;
      if (v != 0.0 && (n_levels == 0 || v > last)) {
        cand = true;
        best = v < best ? v : best;
      }
    }
    best = env_wave_min(best);
    const int flags = (__ballot(cand) ? 1 : 0) | (__ballot(nan) ? 2 : 0);
    __syncthreads();                                       // the partial results of the reduction in front have been read
    if (lane == 0) {
      L.red[wave] = best;
      L.found[wave] = flags;
    }
    __syncthreads();
    int any = 0;
    best = __builtin_huge_val();
#pragma unroll
    for (int k = 0; k < ENV_T / 64; ++k) {
      any |= L.found[k];
      best = L.red[k] < best ? L.red[k] : best;
    }
    if (any & 2) {                                         // (uniform)
      if (tid == 0) status[m] = 3;
      return;
    }
    if (!(any & 1)) break;
    if (n_levels == QTOS_ENV_MAX_LEVELS) {
      if (tid == 0) status[m] = 1;
      return;
    }
    if (tid == 0) L.level[n_levels] = best;
    last = best;
    ++n_levels;
  }
  if (tid == 0) env_seed(L.mt, seed[m]);
  __syncthreads();

  // the draws, the same in every lane: the shifts of the solver's copy (consumed), the map's, then the height passes
  EnvStream S{L.mt, tid, 624, 0};
  S.skip(skip);
  const int n_dir = A.climb ? 2 : 4, k_dir = A.climb ? 2 : 3;
  for (int i = 0; i < A.n_shift; ++i) (void)S.below(n_dir, k_dir);
  int dy = 0, dx = 0;
  for (int i = 0; i < A.n_shift; ++i) {
    const int d = S.below(n_dir, k_dir) + (A.climb ? 2 : 0);   // left, right, up, down
    dx += d == 0 ? -1 : (d == 1 ? 1 : 0);
    dy += d == 2 ? -1 : (d == 3 ? 1 : 0);
  }
  const double lo = -A.delta, width = A.delta - lo;
  const double mine = lane < n_levels ? L.level[lane] : 0.0;
  double v = mine;
  for (int i = 0; i < A.n_height; ++i) env_level_pass(S, v, lane, lo, width);
  v = mine;
  for (int i = 0; i < A.n_height; ++i) env_level_pass(S, v, lane, lo, width);
  if (wave == 0 && lane < n_levels) L.value[lane] = v;
  __syncthreads();

  // the grid, rolled, in both orientations: map_yx[r][c] = moved[r - dy][c - dx] with wrap-around, height_xy[x][y] = map_yx[y][x - 1]
  const int sy = ((dy % rows) + rows) % rows, sx = ((dx % cols) + cols) % cols;
  auto moved = [&](int r, int c) -> double {
    int sr = r - sy, sc = c - sx;
    sr += sr < 0 ? rows : 0;
    sc += sc < 0 ? cols : 0;
    const double h = g[(size_t)sr * cols + sc];
    if (h == 0.0) return h;                                // (ground keeps its own zero, -0.0 included)
    int at = 0;
#pragma unroll
    for (int step = QTOS_ENV_MAX_LEVELS / 2; step > 0; step >>= 1)
      if (at + step < n_levels && L.level[at + step] <= h) at += step;
    return L.value[at];
  };
  double *out = map_yx + (size_t)m * cells;
  for (int ci = tid; ci < cells; ci += ENV_T) out[ci] = moved(ci / cols, ci % cols);
  if (height_xy) {
    double *hx = height_xy + (size_t)m * cells;
    for (int ci = tid; ci < cells; ci += ENV_T) {
      const int x = ci / rows, y = ci % rows;
      hx[ci] = x == 0 ? 0.0 : moved(y, x - 1);
    }
  }
  if (tid == 0) {
    if (draws) draws[m] = skip + S.used;
    status[m] = 0;
  }
}

}  // namespace qtos
