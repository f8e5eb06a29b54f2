// window_api.hpp -- the sampler's and the receding loop's entries of the C ABI (include/qtos_planner.h) over window_kernels.hpp.
// A part of qtos_planner.hip, included inside its extern "C" block, behind the handle (QtosPlanner), HIPCHK and Staging.
//
// A window kernel brings three pieces: X_args, the argument checks of both forms and QtosX as the kernel reads it;
// qtos_X_device, the launch on the caller's stream over device arrays; qtos_X, the host form over host arrays, which states
// its arrays to a Staging (in, out, inout: which are optional, how many elements, which come back), looks at its rc, calls
// the device form on the null stream and downloads.  qtos_handover and qtos_shift_warm go through the handle's own staging
// buffers and stream instead.

int qtos_sample_csv_device(QtosPlanner *p, int B, const double *d_nodes, const double *d_t0, double hz,
                           int n_rows, double *d_rows_out, void *stream_) {
  if (!p || B < 1 || !d_nodes || !d_t0 || !d_rows_out || n_rows < 1 || !(hz > 0)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  dim3 grid((n_rows + 255) / 256, B);
  hipLaunchKernelGGL(k_sample, grid, dim3(256), 0, (hipStream_t)stream_, p->sp, d_nodes, d_t0, hz, n_rows, d_rows_out, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

// The plan as the text file the reference fetches from its container (build/traj.csv -> ./data/traj/towr.csv: scripts/main.py:90-92):
// n_rows x 37 numbers printed like the solver's C++ stream prints them ("%g"), csv_writer.hpp.  Host only, no planner handle.
int qtos_write_csv(const char *path, const double *rows, int n_rows, int n_threads) {
  return write_csv_file(path, rows, n_rows, QTOS_CSV_COLS, n_threads);
}

int qtos_sample_csv(QtosPlanner *p, int B, const double *nodes, const double *t0, double hz, int n_rows, double *rows_out) {
  if (!p || B < 1 || !nodes || !t0 || !rows_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  double *d_rows = S.out(rows_out, (size_t)B * n_rows * QTOS_CSV_COLS);
  if (S.rc) return S.rc;
  const int rc = qtos_sample_csv_device(p, B, d_nodes, d_t0, hz, n_rows, d_rows, nullptr);
  return rc ? rc : S.download();
}

// ---- time-shifted warm start (receding-horizon replans) ---------------------------------------------
// Every variable of the new plan sits at a node time t; where the previous plan still covers offset + t its
// spline is evaluated there (positions / velocities / forces in the common world frame), beyond its horizon
// the straight-line guess of the new problem takes over; fixed variables carry the new start / goal.
__global__ __launch_bounds__(256) void k_shift_warm(DevPlan P, SamplePlan S, const double *prev, const double *offset,
                                                    const double *start, const double *goal, const int *map_id, double *out, int B) {
  const int b = blockIdx.x;
  if (b >= B) return;
  const double *x = prev + (size_t)b * P.n_vars, *st = start + (size_t)b * QTOS_START_DOUBLES, *gl = goal + (size_t)b * 3;
  const int map = map_id ? map_id[b] : 0;
  const double off = offset[b];
  for (int v = threadIdx.x; v < P.n_vars; v += blockDim.x) {
    const InitDesc I = P.init[v];
    double val;
    if (I.fix_src >= 0) val = I.fix_src < 24 ? st[I.fix_src] : (I.fix_src < 26 ? gl[I.fix_src - 24] : 0.0);
    else {
      const double t = off + P.var_time[v];
      if (t <= S.T + 1e-9) {
        // (picked with constant indices: an index into the splines of the kernel arguments copies all of them to scratch)
        SampleSpline sp = S.lin;
        if (I.set == 1) sp = S.ang;
#pragma unroll
        for (int e = 0; e < NEE; ++e) {
          if (I.set == 2 + e) sp = S.eem[e];
          if (I.set == 6 + e) sp = S.eef[e];
        }
        double o3[3];
        sample_spline<true>(sp, x, fmin(t, S.T), I.is_vel, o3);
        val = o3[I.dim];
      } else val = straight_line_value(P, I, st, gl, map);
    }
    out[(size_t)b * P.n_vars + v] = val;
  }
}

int qtos_shift_warm_device(QtosPlanner *p, int B, const double *d_nodes_prev, const double *d_offset, const double *d_start,
                           const double *d_goal, const int *d_map_id, double *d_warm_out, void *stream_) {
  if (!p || B < 1 || !d_nodes_prev || !d_offset || !d_start || !d_goal || !d_warm_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_shift_warm, dim3(B), dim3(256), 0, (hipStream_t)stream_, p->dp, p->sp, d_nodes_prev, d_offset, d_start, d_goal,
                     d_map_id, d_warm_out, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_shift_warm(QtosPlanner *p, int B, const double *nodes_prev, const double *offset, const double *start, const double *goal,
                    const int *map_id, double *warm_out) {
  if (!p || B < 1 || B > p->max_batch || !nodes_prev || !offset || !start || !goal || !warm_out) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t n = p->M.n_vars;
  hipStream_t st = p->own_stream;
  double *d_off = nullptr;
  HIPCHK(p, hipMalloc((void **)&d_off, B * sizeof(double)));
  hipError_t e = hipSuccess;
  auto cp = [&](void *dst, const void *src, size_t bytes, hipMemcpyKind k) { if (e == hipSuccess) e = hipMemcpyAsync(dst, src, bytes, k, st); };
  cp(p->d_nodes, nodes_prev, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice);
  cp(d_off, offset, B * sizeof(double), hipMemcpyHostToDevice);
  cp(p->d_start, start, (size_t)B * QTOS_START_DOUBLES * sizeof(double), hipMemcpyHostToDevice);
  cp(p->d_goal, goal, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice);
  if (map_id) cp(p->d_map, map_id, B * sizeof(int), hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? qtos_shift_warm_device(p, B, p->d_nodes, d_off, p->d_start, p->d_goal, map_id ? p->d_map : nullptr, p->d_warm, (void *)st) : -2;
  if (!rc) {
    cp(warm_out, p->d_warm, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = -2;
  }
  (void)hipFree(d_off);
  return rc;
}

// ---- hand-over of a replan (k_handover, window_kernels.hpp) --------------------------------------------------
// The argument checks of both forms, and QtosHandover as k_handover reads it.
static int handover_args(const QtosPlanner *p, int B, const QtosHandover *h, const void *nodes, const void *goal_step, const void *start_out,
                         const void *goal_out, const void *offset_out, HandoverArgs *H) {
  if (!p || B < 1 || !h || !nodes || !start_out || !offset_out || (goal_step == nullptr) != (goal_out == nullptr)) return -1;
  if (h->rule != 0 && h->rule != 1) return -1;
  if (h->rule == 1 && (h->n_heights < 1 || h->n_heights > 8)) return -1;
  if (!(h->advance >= 0) || !(h->search >= 0)) return -1;
  H->hz = h->hz > 0 ? h->hz : 1000.0;
  const double last = std::round(p->M.T * H->hz), a = std::round(h->advance * H->hz), s = std::round(h->search * H->hz);
  if (a > last || s > 1e6) return -1;
  H->k0 = (int)a;
  H->n_search = (int)s;
  H->rule = h->rule; H->zero_filter = h->zero_filter != 0; H->turn = h->turn != 0;
  H->x_lo = h->x_lo; H->x_hi = h->x_hi;
  for (int j = 0; j < 8; ++j) H->h6[j] = h->rule == 1 && j < h->n_heights ? std::rint(h->heights[j] * 1e6) : NAN;
  return 0;
}

static int handover_launch(QtosPlanner *p, int B, const HandoverArgs &H, const double *d_nodes, double *d_goal_step, double *d_start_out,
                           double *d_goal_out, double *d_offset_out, int *d_row_out, hipStream_t st) {
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_handover, dim3(B), dim3(512), 0, st, p->d_sp, H, d_nodes, d_goal_step, d_start_out, d_goal_out, d_offset_out,
                     d_row_out, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_handover_device(QtosPlanner *p, int B, const QtosHandover *h, const double *d_nodes, double *d_goal_step, double *d_start_out,
                         double *d_goal_out, double *d_offset_out, int *d_row_out, void *stream_) {
  HandoverArgs H;
  if (handover_args(p, B, h, d_nodes, d_goal_step, d_start_out, d_goal_out, d_offset_out, &H)) return -1;
  return handover_launch(p, B, H, d_nodes, d_goal_step, d_start_out, d_goal_out, d_offset_out, d_row_out, (hipStream_t)stream_);
}

int qtos_handover(QtosPlanner *p, int B, const QtosHandover *h, const double *nodes, double *goal_step, double *start_out, double *goal_out,
                  double *offset_out, int *row_out) {
  HandoverArgs H;
  if (handover_args(p, B, h, nodes, goal_step, start_out, goal_out, offset_out, &H) || B > p->max_batch) return -1;
  if (p->call_open || p->busy.load()) { p->err = "qtos_handover: a call is open (the host form goes through the handle's staging buffers)"; return -5; }
  HIPCHK(p, hipSetDevice(p->device));
  const size_t n = p->M.n_vars;
  hipStream_t st = p->own_stream;
  // staging: nodes, start and goal in their own buffers; goal step (3 B doubles), offset (B) and row (B ints) in the warm-start
  // buffer: max_batch x n_vars doubles, and 5 B doubles are used -- a plan has hundreds of variables, checked all the same
  if (n < 5) { p->err = "qtos_handover: the staging buffer is too small"; return -1; }
  double *d_gs = p->d_warm, *d_off = p->d_warm + 3 * (size_t)B;
  int *d_row = (int *)(p->d_warm + 4 * (size_t)B);
  HIPCHK(p, hipMemcpyAsync(p->d_nodes, nodes, (size_t)B * n * sizeof(double), hipMemcpyHostToDevice, st));
  if (goal_step) {
    HIPCHK(p, hipMemcpyAsync(d_gs, goal_step, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    HIPCHK(p, hipMemcpyAsync(p->d_goal, goal_out, (size_t)B * 3 * sizeof(double), hipMemcpyHostToDevice, st));   // (goal_out[b][2] stays the caller's)
  }
  int rc = handover_launch(p, B, H, p->d_nodes, goal_step ? d_gs : nullptr, p->d_start, goal_step ? p->d_goal : nullptr, d_off, d_row, st);
  if (rc) return rc;
  HIPCHK(p, hipMemcpyAsync(start_out, p->d_start, (size_t)B * QTOS_START_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, st));
  HIPCHK(p, hipMemcpyAsync(offset_out, d_off, B * sizeof(double), hipMemcpyDeviceToHost, st));
  if (row_out) HIPCHK(p, hipMemcpyAsync(row_out, d_row, B * sizeof(int), hipMemcpyDeviceToHost, st));
  if (goal_step) {
    HIPCHK(p, hipMemcpyAsync(goal_step, d_gs, (size_t)B * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(p, hipMemcpyAsync(goal_out, p->d_goal, (size_t)B * 3 * sizeof(double), hipMemcpyDeviceToHost, st));
  }
  HIPCHK(p, hipStreamSynchronize(st));
  return 0;
}

// ---- stitching of receding windows (k_stitch, window_kernels.hpp) ----------------------------------------------
// The argument checks of both forms, and QtosStitch as k_stitch reads it.
static int stitch_args(const QtosPlanner *p, int B, const QtosStitch *s, const void *nodes, const void *n_rows, const void *t0,
                       const void *traj, const void *cursor, StitchArgs *A) {
  if (!p || B < 1 || !s || !nodes || !t0 || !traj || !cursor) return -1;
  if (s->capacity < 1 || segment_check(s->capacity, s->n_rows, s->first_row, true, !n_rows)) return -1;   // (always a ring)
  A->hz = s->hz > 0 ? s->hz : 1000.0;
  A->capacity = s->capacity;
  A->first_row = s->first_row; A->n_rows = s->n_rows; A->advance_clock = s->advance_clock != 0;
  return 0;
}

int qtos_stitch_device(QtosPlanner *p, int B, const QtosStitch *s, const double *d_nodes, const int *d_n_rows, double *d_t0,
                       double *d_traj, long long *d_cursor, void *stream_) {
  StitchArgs A;
  if (stitch_args(p, B, s, d_nodes, d_n_rows, d_t0, d_traj, d_cursor, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_stitch, dim3(B), dim3(STITCH_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_n_rows, d_t0, d_traj,
                     d_cursor, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_stitch(QtosPlanner *p, int B, const QtosStitch *s, const double *nodes, const int *n_rows, double *t0, double *traj,
                long long *cursor) {
  StitchArgs A;
  if (stitch_args(p, B, s, nodes, n_rows, t0, traj, cursor, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars);
  const int *d_n = S.in(n_rows, B);
  double *d_t0 = S.inout(t0, B), *d_traj = S.inout(traj, segment_elems(B, A.capacity, A.n_rows) * QTOS_CSV_COLS);
  long long *d_cur = S.inout(cursor, B);
  if (S.rc) return S.rc;
  const int rc = qtos_stitch_device(p, B, s, d_nodes, d_n, d_t0, d_traj, d_cur, nullptr);
  return rc ? rc : S.download();
}

// ---- joint commands of the windows' plans (k_joint_rows, window_kernels.hpp) -----------------------------------
// The argument checks of both forms, and QtosJointRows as k_joint_rows reads it.
static int joint_args(const QtosPlanner *p, int B, const QtosJointRows *s, const void *nodes, const void *t0, const void *first_row,
                      const void *n_rows, const void *cursor, const void *q_mes, const void *qd_mes, const void *out,
                      const void *status, JointArgs *A) {
  (void)first_row; (void)n_rows;
  if (!p || B < 1 || !s || !nodes || !t0 || !out || !status) return -1;
  if (segment_check(s->capacity, s->n_rows, s->first_row, cursor != nullptr) || (q_mes == nullptr) != (qd_mes == nullptr)) return -1;
  if (!(s->l_upper > 0) || !(s->l_lower > 0)) return -1;
  A->hz = s->hz > 0 ? s->hz : 1000.0;
  A->ee_shift = s->ee_shift; A->l_upper = s->l_upper; A->l_lower = s->l_lower; A->tau_max = s->tau_max;
  for (int e = 0; e < NEE; ++e) {
    for (int d = 0; d < 3; ++d) A->hip[e][d] = s->hip[e][d];
    A->lateral[e] = s->lateral[e]; A->knee_sign[e] = s->knee_sign[e];
  }
  for (int j = 0; j < 3 * NEE; ++j) { A->kp[j] = s->kp[j]; A->kd[j] = s->kd[j]; }
  A->capacity = s->capacity; A->first_row = s->first_row; A->n_rows = s->n_rows; A->flags = s->flags;
  return 0;
}

int qtos_joint_rows_device(QtosPlanner *p, int B, const QtosJointRows *s, const double *d_nodes, const double *d_t0,
                           const int *d_first_row, const int *d_n_rows, const long long *d_cursor, const double *d_q_mes,
                           const double *d_qd_mes, double *d_out, int *d_status, void *stream_) {
  JointArgs A;
  if (joint_args(p, B, s, d_nodes, d_t0, d_first_row, d_n_rows, d_cursor, d_q_mes, d_qd_mes, d_out, d_status, &A)) return -1;
  const long long most = most_rows(A.capacity, A.n_rows, d_n_rows != nullptr);
  if (most < 1) return 0;
  const int lanes = most > JOINT_TICK ? JOINT_TILE : JOINT_TICK;
  const long long tiles = (most + lanes - 1) / lanes;
  if (tiles > 65535 || B > 65535) { p->err = "qtos_joint_rows: too many rows or windows for one launch"; return -1; }
  HIPCHK(p, hipSetDevice(p->device));
  if (lanes == JOINT_TILE)
    hipLaunchKernelGGL(k_joint_rows<JOINT_TILE>, dim3((unsigned)tiles, B), dim3(JOINT_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes,
                       d_t0, d_first_row, d_n_rows, d_cursor, d_q_mes, d_qd_mes, d_out, d_status, B);
  else
    hipLaunchKernelGGL(k_joint_rows<JOINT_TICK>, dim3((unsigned)tiles, B), dim3(JOINT_TICK), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes,
                       d_t0, d_first_row, d_n_rows, d_cursor, d_q_mes, d_qd_mes, d_out, d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_joint_rows(QtosPlanner *p, int B, const QtosJointRows *s, const double *nodes, const double *t0, const int *first_row,
                    const int *n_rows, const long long *cursor, const double *q_mes, const double *qd_mes, double *out, int *status) {
  JointArgs A;
  if (joint_args(p, B, s, nodes, t0, first_row, n_rows, cursor, q_mes, qd_mes, out, status, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.capacity, A.n_rows);
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  double *d_out = S.inout(out, rows * QTOS_CSV_COLS);
  int *d_st = S.inout(status, rows);
  const int *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_qm = S.in(q_mes, (size_t)B * 3 * NEE), *d_qdm = S.in(qd_mes, (size_t)B * 3 * NEE);
  if (S.rc) return S.rc;
  const int rc = qtos_joint_rows_device(p, B, s, d_nodes, d_t0, d_first, d_n, d_cur, d_qm, d_qdm, d_out, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- measured states and tracking errors of the windows (k_track, window_kernels.hpp) ---------------------------
// The argument checks of both forms, and QtosTrack as k_track reads it.
static int track_args(const QtosPlanner *p, int B, const QtosTrack *s, const void *nodes, const void *t0, const void *cursor,
                      const void *meas, const void *count, const void *total, const void *out, const void *status, TrackArgs *A) {
  if (!p || B < 1 || !s || !nodes || !t0 || !meas || !count || !total || !out || !status) return -1;
  if (segment_check(s->capacity, s->n_rows, s->first_row, cursor != nullptr) || s->delay < 0) return -1;
  if (!(s->l_upper > 0) || !(s->l_lower > 0)) return -1;
  A->hz = s->hz > 0 ? s->hz : 1000.0;
  A->ee_shift = s->ee_shift; A->l_upper = s->l_upper; A->l_lower = s->l_lower;
  for (int e = 0; e < NEE; ++e) {
    for (int d = 0; d < 3; ++d) A->hip[e][d] = s->hip[e][d];
    A->lateral[e] = s->lateral[e];
  }
  A->capacity = s->capacity; A->first_row = s->first_row; A->n_rows = s->n_rows; A->delay = s->delay; A->flags = s->flags;
  return 0;
}

int qtos_track_device(QtosPlanner *p, int B, const QtosTrack *s, const double *d_nodes, const double *d_t0, const int *d_first_row,
                      const int *d_n_rows, const long long *d_cursor, const double *d_meas, const double *d_goal_x, long long *d_count,
                      double *d_total, double *d_out, int *d_status, void *stream_) {
  TrackArgs A;
  if (track_args(p, B, s, d_nodes, d_t0, d_cursor, d_meas, d_count, d_total, d_out, d_status, &A)) return -1;
  const long long most = most_rows(A.capacity, A.n_rows, d_n_rows != nullptr);
  if (most < 1) return 0;
  HIPCHK(p, hipSetDevice(p->device));
  if (most > TRACK_TICK)
    hipLaunchKernelGGL(k_track<TRACK_TILE>, dim3(B), dim3(TRACK_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_first_row,
                       d_n_rows, d_cursor, d_meas, d_goal_x, d_count, d_total, d_out, d_status, B);
  else
    hipLaunchKernelGGL(k_track<TRACK_TICK>, dim3(B), dim3(TRACK_TICK), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_first_row,
                       d_n_rows, d_cursor, d_meas, d_goal_x, d_count, d_total, d_out, d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_track(QtosPlanner *p, int B, const QtosTrack *s, const double *nodes, const double *t0, const int *first_row, const int *n_rows,
               const long long *cursor, const double *meas, const double *goal_x, long long *count, double *total, double *out,
               int *status) {
  TrackArgs A;
  if (track_args(p, B, s, nodes, t0, cursor, meas, count, total, out, status, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.capacity, A.n_rows);
  const size_t mcols = (A.flags & QTOS_TRACK_QUAT) ? 19 : 18;
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B), *d_meas = S.in(meas, rows * mcols);
  double *d_out = S.inout(out, rows * TRACK_COLS);
  int *d_st = S.inout(status, rows);
  long long *d_count = S.inout(count, (size_t)B * 2);
  double *d_total = S.inout(total, (size_t)B * 2);
  const int *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_goal = S.in(goal_x, B);
  if (S.rc) return S.rc;
  const int rc = qtos_track_device(p, B, s, d_nodes, d_t0, d_first, d_n, d_cur, d_meas, d_goal, d_count, d_total, d_out, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- feedback hand-over: the next plan starts from the measured state (k_start_feedback, window_kernels.hpp) ------
// The argument checks of both forms, and QtosFeedback as k_start_feedback reads it.
static int feedback_args(const QtosPlanner *p, int B, const QtosFeedback *s, const void *nodes, const void *t0, const void *row,
                         const void *cursor, const void *meas, const void *start, const void *goal_step, const void *goal,
                         const void *status, FeedbackArgs *A) {
  if (!p || B < 1 || !s || !nodes || !t0 || !row || !meas || !start || !status || (goal_step == nullptr) != (goal == nullptr)) return -1;
  if (segment_check(s->capacity, s->n_rows, s->first_row, cursor != nullptr, false) || !(s->latency >= 0)) return -1;   // (one row: no count)
  if (!(s->l_upper > 0) || !(s->l_lower > 0)) return -1;
  for (double g : {s->gain_pos, s->gain_ang, s->gain_foot})
    if (!(g >= 0 && g <= 1)) return -1;
  if (!(s->max_pos > 0) || !(s->max_ang > 0) || !(s->max_foot > 0)) return -1;
  TrackArgs &K = A->K;
  K.hz = s->hz > 0 ? s->hz : 1000.0;
  K.ee_shift = s->ee_shift; K.l_upper = s->l_upper; K.l_lower = s->l_lower;
  for (int e = 0; e < NEE; ++e) {
    for (int d = 0; d < 3; ++d) { K.hip[e][d] = s->hip[e][d]; A->nominal[e][d] = s->nominal[e][d]; }
    K.lateral[e] = s->lateral[e];
  }
  K.capacity = s->capacity; K.first_row = s->first_row; K.n_rows = s->n_rows; K.delay = 0;
  K.flags = (s->flags & QTOS_FEEDBACK_QUAT) ? 1 : 0;
  const double lat = std::round(s->latency * K.hz);
  A->lat = lat > 2e9 ? 2000000000 : (int)lat;
  A->gain_pos = s->gain_pos; A->gain_ang = s->gain_ang; A->gain_foot = s->gain_foot;
  A->max_pos = s->max_pos; A->max_ang = s->max_ang; A->max_foot = s->max_foot;
  for (int d = 0; d < 3; ++d) A->max_deviation[d] = s->max_deviation[d];
  A->rom_tol = s->rom_tol; A->snap_tol = s->snap_tol;
  A->snap = (s->flags & QTOS_FEEDBACK_SNAP) != 0; A->zero_filter = (s->flags & QTOS_FEEDBACK_ZERO_FILTER) != 0;
  const DevPlan &D = p->dp;
  A->T.height = D.height; A->T.hcell = D.hcell; A->T.hx0 = D.hx0; A->T.hy0 = D.hy0;
  A->T.n_maps = D.n_maps; A->T.hnx = D.hnx; A->T.hny = D.hny; A->T.terrain_mode = D.terrain_mode;
  return 0;
}

int qtos_start_feedback_device(QtosPlanner *p, int B, const QtosFeedback *s, const double *d_nodes, const double *d_t0, const int *d_row,
                               const long long *d_cursor, const double *d_meas, const int *d_map_id, double *d_start,
                               const double *d_goal_step, double *d_goal, double *d_err_out, int *d_status, void *stream_) {
  FeedbackArgs A;
  if (feedback_args(p, B, s, d_nodes, d_t0, d_row, d_cursor, d_meas, d_start, d_goal_step, d_goal, d_status, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_start_feedback, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_row, d_cursor,
                     d_meas, d_map_id, d_start, d_goal_step, d_goal, d_err_out, d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_start_feedback(QtosPlanner *p, int B, const QtosFeedback *s, const double *nodes, const double *t0, const int *row,
                        const long long *cursor, const double *meas, const int *map_id, double *start, const double *goal_step,
                        double *goal, double *err_out, int *status) {
  FeedbackArgs A;
  if (feedback_args(p, B, s, nodes, t0, row, cursor, meas, start, goal_step, goal, status, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.K.capacity, A.K.n_rows);
  const size_t mcols = A.K.flags ? 19 : 18;
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_row = S.in(row, B);
  const double *d_meas = S.in(meas, rows * mcols);
  double *d_start = S.inout(start, (size_t)B * QTOS_START_DOUBLES);
  int *d_st = S.inout(status, B);
  const long long *d_cur = S.in(cursor, B);
  const int *d_map = S.in(map_id, B);
  const double *d_gs = S.in(goal_step, (size_t)B * 3);
  double *d_goal = S.inout(goal, (size_t)B * 3), *d_err = S.inout(err_out, (size_t)B * 18);
  if (S.rc) return S.rc;
  const int rc = qtos_start_feedback_device(p, B, s, d_nodes, d_t0, d_row, d_cur, d_meas, d_map, d_start, d_gs, d_goal, d_err, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- what the windows' plans violate between their knots (k_plan_check, window_kernels.hpp) --------------------
// The argument checks of both forms, and QtosPlanCheck as k_plan_check reads it, with the model's constants and the terrain.
static_assert(sizeof(CheckRecord) == sizeof(QtosCheckRecord), "QtosCheckRecord (qtos_planner.h) is k_plan_check's record");
static int plan_check_args(const QtosPlanner *p, int B, const QtosPlanCheck *c, const void *nodes, const void *t0, const void *rows,
                           const void *summary, CheckArgs *A) {
  if (!p || B < 1 || !c || !nodes || !t0 || (!rows && !summary)) return -1;
  if (c->n_rows < 1 || c->first_row < 0 || c->first_row > 1000000) return -1;
  const QtosParams &P = p->M.P;
  A->hz = c->hz > 0 ? c->hz : 1000.0;
  A->mass = P.mass; A->gravity = P.gravity; A->mu = P.mu; A->f_max = P.f_max;
  for (int i = 0; i < 9; ++i) A->Ib[i] = P.inertia_b[i];
  for (int e = 0; e < NEE; ++e) {
    for (int d = 0; d < 3; ++d) {
      A->rom_lo[e][d] = P.nominal_stance[e][d] - P.max_dev[d];
      A->rom_hi[e][d] = P.nominal_stance[e][d] + P.max_dev[d];
    }
    A->stance[e] = p->d_stance[e];
  }
  for (int f = 0; f < CHECK_FAMILIES; ++f) A->tol[f] = c->tol[f];
  const DevPlan &D = p->dp;
  A->T.height = D.height; A->T.hcell = D.hcell; A->T.hx0 = D.hx0; A->T.hy0 = D.hy0;
  A->T.n_maps = D.n_maps; A->T.hnx = D.hnx; A->T.hny = D.hny; A->T.terrain_mode = D.terrain_mode;
  A->first_row = c->first_row; A->n_rows = c->n_rows; A->accumulate = (c->flags & QTOS_CHECK_ACCUMULATE) != 0;
  return 0;
}

int qtos_plan_check_device(QtosPlanner *p, int B, const QtosPlanCheck *c, const double *d_nodes, const double *d_t0, const int *d_map_id,
                           const int *d_first_row, const int *d_n_rows, const long long *d_cursor, double *d_rows,
                           QtosCheckRecord *d_summary, void *stream_) {
  CheckArgs A;
  if (plan_check_args(p, B, c, d_nodes, d_t0, d_rows, d_summary, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_plan_check, dim3(B), dim3(CHECK_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_map_id, d_first_row,
                     d_n_rows, d_cursor, d_rows, (CheckRecord *)d_summary, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_plan_check(QtosPlanner *p, int B, const QtosPlanCheck *c, const double *nodes, const double *t0, const int *map_id,
                    const int *first_row, const int *n_rows, const long long *cursor, double *rows, QtosCheckRecord *summary) {
  CheckArgs A;
  if (plan_check_args(p, B, c, nodes, t0, rows, summary, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_map = S.in(map_id, B), *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  double *d_rows = S.inout(rows, (size_t)B * (size_t)c->n_rows * CHECK_COLS);    // (rows behind a window's count come back as they were)
  QtosCheckRecord *d_sum = S.inout(summary, (size_t)B * CHECK_FAMILIES);          // (the accumulate flag merges with what is there)
  if (S.rc) return S.rc;
  const int rc = qtos_plan_check_device(p, B, c, d_nodes, d_t0, d_map, d_first, d_n, d_cur, d_rows, d_sum, nullptr);
  return rc ? rc : S.download();
}

// ---- the windows' robots as simulated rigid bodies (k_rollout, window_kernels.hpp) -----------------------------
// The argument checks of both forms, and QtosRollout as k_rollout reads it.  Every -1 but the null planner's leaves its reason in
// the handle's err.
static int rollout_args(QtosPlanner *p, int B, const QtosRollout *s, const void *nodes, const void *t0, const void *cursor,
                        const void *state, const void *count, const void *word, const void *meas, const void *status, RolloutArgs *A) {
  if (!p) return -1;
  const char *why = nullptr;
  if (B < 1) why = "B < 1";
  else if (!s || !nodes || !t0 || !state || !count || !word || !meas || !status) why = "a required pointer is null";
  else if (const char *seg = segment_check(s->capacity, s->n_rows, s->first_row, cursor != nullptr)) why = seg;
  else if (s->substeps < 1 || s->substeps > 1000) why = "substeps is 1 .. 1000";
  else if (!(s->hz > 0) || !(s->hz <= 1e9)) why = "hz is > 0";
  else if (!(s->mass > 0) || !(s->mass <= 1.7976931348623157e308)) why = "mass is > 0";
  else if (s->push_from < 0 || s->push_ticks < 0) why = "push_from and push_ticks are >= 0";
  if (!why) {
    const double *a = s->inertia_b;
    const double det = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6]);
    double big = 0;
    bool finite = std::isfinite(det);
    for (int i = 0; i < 9; ++i) {
      big = std::max(big, std::fabs(a[i]));
      finite = finite && std::isfinite(a[i]) && std::isfinite(s->inertia_b_inv[i]);
    }
    if (!finite || !(std::fabs(det) > 1e-12 * big * big * big)) why = "inertia_b is singular (or it or inertia_b_inv is not finite)";
  }
  if (why) {
    p->err = std::string("qtos_rollout: ") + why;
    return -1;
  }
  A->hz = s->hz; A->h = 1.0 / (s->hz * (double)s->substeps);
  A->mass = s->mass; A->gravity = s->gravity; A->ff_scale = s->ff_scale;
  A->f_fb_max = s->f_fb_max; A->t_fb_max = s->t_fb_max; A->dev_max = s->dev_max; A->tilt_max = s->tilt_max;
  for (int i = 0; i < 9; ++i) { A->Ib[i] = s->inertia_b[i]; A->Ii[i] = s->inertia_b_inv[i]; }
  for (int i = 0; i < 3; ++i) {
    A->kp_lin[i] = s->kp_lin[i]; A->kd_lin[i] = s->kd_lin[i]; A->kp_ang[i] = s->kp_ang[i]; A->kd_ang[i] = s->kd_ang[i];
  }
  A->capacity = s->capacity; A->push_from = s->push_from; A->push_ticks = s->push_ticks;
  A->first_row = s->first_row; A->n_rows = s->n_rows; A->substeps = s->substeps; A->flags = s->flags;
  return 0;
}

int qtos_rollout_device(QtosPlanner *p, int B, const QtosRollout *s, const double *d_nodes, const double *d_t0, const int *d_first_row,
                        const int *d_n_rows, const long long *d_cursor, const double *d_joint, const double *d_mass_scale,
                        const double *d_push, double *d_state, long long *d_count, int *d_word, double *d_meas, double *d_rows,
                        int *d_status, void *stream_) {
  RolloutArgs A;
  if (rollout_args(p, B, s, d_nodes, d_t0, d_cursor, d_state, d_count, d_word, d_meas, d_status, &A)) return -1;
  const long long most = most_rows(A.capacity, A.n_rows, d_n_rows != nullptr);
  if (most < 1) return 0;
  HIPCHK(p, hipSetDevice(p->device));
  if (most > ROLLOUT_TICK)
    hipLaunchKernelGGL(k_rollout<ROLLOUT_TILE>, dim3(B), dim3(ROLLOUT_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_first_row,
                       d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_status, B);
  else
    hipLaunchKernelGGL(k_rollout<ROLLOUT_TICK>, dim3(B), dim3(ROLLOUT_TICK), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_first_row,
                       d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_rollout(QtosPlanner *p, int B, const QtosRollout *s, const double *nodes, const double *t0, const int *first_row,
                 const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                 double *state, long long *count, int *word, double *meas, double *rows_out, int *status) {
  RolloutArgs A;
  if (rollout_args(p, B, s, nodes, t0, cursor, state, count, word, meas, status, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.capacity, A.n_rows);
  const size_t mcols = (A.flags & QTOS_ROLLOUT_QUAT) ? 19 : 18;
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_joint = S.in(joint, rows * QTOS_CSV_COLS), *d_ms = S.in(mass_scale, B), *d_push = S.in(push, (size_t)B * 6);
  double *d_state = S.inout(state, (size_t)B * 13);
  long long *d_count = S.inout(count, B);
  int *d_word = S.inout(word, B);
  double *d_meas = S.inout(meas, rows * mcols), *d_rows = S.inout(rows_out, rows * ROLLOUT_COLS);
  int *d_st = S.inout(status, rows);
  if (S.rc) return S.rc;
  const int rc = qtos_rollout_device(p, B, s, d_nodes, d_t0, d_first, d_n, d_cur, d_joint, d_ms, d_push, d_state, d_count, d_word, d_meas,
                                     d_rows, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- the rollout with its feedback through the stance feet (k_rollout_feet, window_kernels.hpp) ------------------
// The argument checks of both forms: qtos_rollout's on the body (the structure's first sizeof(QtosRollout) bytes), then the feet's own; QtosRolloutFeet as k_rollout_feet reads it.
static int rollout_feet_args(QtosPlanner *p, int B, const QtosRolloutFeet *s, const void *nodes, const void *t0, const void *cursor,
                             const void *state, const void *count, const void *word, const void *meas, const void *status, RolloutArgs *A,
                             FeetArgs *F) {
  if (!p) return -1;
  if (!s) {
    p->err = "qtos_rollout_feet: a required pointer is null";
    return -1;
  }
  static_assert(offsetof(QtosRolloutFeet, arm) == sizeof(QtosRollout) && offsetof(QtosRolloutFeet, push_ticks) == offsetof(QtosRollout, push_ticks) &&
                    offsetof(QtosRolloutFeet, flags) == offsetof(QtosRollout, flags) && offsetof(QtosRolloutFeet, ff_scale) == offsetof(QtosRollout, ff_scale),
                "QtosRolloutFeet begins with QtosRollout's fields");
  QtosRollout body;
  std::memcpy(&body, s, sizeof(body));
  if (rollout_args(p, B, &body, nodes, t0, cursor, state, count, word, meas, status, A)) {
    p->err = "qtos_rollout_feet: " + p->err.substr(p->err.find(": ") + 2);
    return -1;
  }
  const char *why = nullptr;
  if (!(s->arm > 0) || !(s->arm <= 1.7976931348623157e308)) why = "arm is > 0";
  else if (!(s->damping > 0) || !(s->damping <= 1.7976931348623157e308)) why = "damping is > 0";
  else if (!(s->w_min > 0) || !(s->w_min <= 1)) why = "w_min is in (0, 1]";
  else if (!(s->mu >= 0)) why = "mu is >= 0";
  if (why) {
    p->err = std::string("qtos_rollout_feet: ") + why;
    return -1;
  }
  F->arm = s->arm; F->damping = s->damping; F->w_min = s->w_min; F->mu = s->mu; F->f_max = s->f_max;
  for (int e = 0; e < NEE; ++e) F->stance[e] = p->d_stance[e];
  F->limit = (s->feet_flags & QTOS_FEET_LIMIT) != 0;
  return 0;
}

int qtos_rollout_feet_device(QtosPlanner *p, int B, const QtosRolloutFeet *s, const double *d_nodes, const double *d_t0,
                             const int *d_first_row, const int *d_n_rows, const long long *d_cursor, const double *d_joint,
                             const double *d_mass_scale, const double *d_push, double *d_state, long long *d_count, int *d_word,
                             double *d_meas, double *d_rows, double *d_frows, int *d_status, void *stream_) {
  RolloutArgs A;
  FeetArgs F;
  if (rollout_feet_args(p, B, s, d_nodes, d_t0, d_cursor, d_state, d_count, d_word, d_meas, d_status, &A, &F)) return -1;
  const long long most = most_rows(A.capacity, A.n_rows, d_n_rows != nullptr);
  if (most < 1) return 0;
  HIPCHK(p, hipSetDevice(p->device));
  if (most > ROLLOUT_TICK)
    hipLaunchKernelGGL(k_rollout_feet<ROLLOUT_TILE>, dim3(B), dim3(ROLLOUT_TILE), 0, (hipStream_t)stream_, p->d_sp, A, F, d_nodes, d_t0,
                       d_first_row, d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_frows,
                       d_status, B);
  else
    hipLaunchKernelGGL(k_rollout_feet<ROLLOUT_TICK>, dim3(B), dim3(ROLLOUT_TICK), 0, (hipStream_t)stream_, p->d_sp, A, F, d_nodes, d_t0,
                       d_first_row, d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_frows,
                       d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_rollout_feet(QtosPlanner *p, int B, const QtosRolloutFeet *s, const double *nodes, const double *t0, const int *first_row,
                      const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                      double *state, long long *count, int *word, double *meas, double *rows_out, double *frows, int *status) {
  RolloutArgs A;
  FeetArgs F;
  if (rollout_feet_args(p, B, s, nodes, t0, cursor, state, count, word, meas, status, &A, &F)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.capacity, A.n_rows);
  const size_t mcols = (A.flags & QTOS_ROLLOUT_QUAT) ? 19 : 18;
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_joint = S.in(joint, rows * QTOS_CSV_COLS), *d_ms = S.in(mass_scale, B), *d_push = S.in(push, (size_t)B * 6);
  double *d_state = S.inout(state, (size_t)B * 13);
  long long *d_count = S.inout(count, B);
  int *d_word = S.inout(word, B);
  double *d_meas = S.inout(meas, rows * mcols), *d_rows = S.inout(rows_out, rows * ROLLOUT_COLS), *d_frows = S.inout(frows, rows * FEET_COLS);
  int *d_st = S.inout(status, rows);
  if (S.rc) return S.rc;
  const int rc = qtos_rollout_feet_device(p, B, s, d_nodes, d_t0, d_first, d_n, d_cur, d_joint, d_ms, d_push, d_state, d_count, d_word,
                                          d_meas, d_rows, d_frows, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- the rows' contact forces fitted to the planned motion (k_force_fit, window_kernels.hpp) ---------------------
// The argument checks of both forms, and QtosForceFit as k_force_fit reads it, with the model's constants and the terrain.  Every
// -1 but the null planner's leaves its reason in the handle's err.
static int force_fit_args(QtosPlanner *p, int B, const QtosForceFit *s, const void *nodes, const void *t0, const void *cursor,
                          const void *rows, const void *status, const void *summary, FitArgs *A) {
  if (!p) return -1;
  const char *why = nullptr;
  if (B < 1) why = "B < 1";
  else if (!s || !nodes || !t0) why = "a required pointer is null";
  else if ((rows == nullptr) != (status == nullptr)) why = "rows and status go together";
  else if (!rows && !summary) why = "rows and summary are both null";
  else if (const char *seg = segment_check(s->capacity, s->n_rows, s->first_row, cursor != nullptr)) why = seg;
  else if (!(s->arm > 0) || !(s->arm <= 1.7976931348623157e308)) why = "arm is > 0";
  else if (!(s->damping > 0) || !(s->damping <= 1.7976931348623157e308)) why = "damping is > 0";
  else if (!(s->w_min > 0) || !(s->w_min <= 1)) why = "w_min is in (0, 1]";
  else if (s->excess_tol != s->excess_tol) why = "excess_tol is not a number";
  else if (!(s->l_upper > 0) || !(s->l_lower > 0)) why = "a link length is <= 0";
  if (why) {
    p->err = std::string("qtos_force_fit: ") + why;
    return -1;
  }
  const QtosParams &P = p->M.P;
  A->hz = s->hz > 0 ? s->hz : 1000.0;
  A->mass = P.mass; A->gravity = P.gravity; A->mu = P.mu; A->f_max = P.f_max;
  for (int i = 0; i < 9; ++i) A->Ib[i] = P.inertia_b[i];
  A->arm = s->arm; A->damping = s->damping; A->w_min = s->w_min; A->excess_tol = s->excess_tol;
  for (int f = 0; f < FIT_FAMILIES; ++f) A->tol[f] = s->tol[f];
  for (int e = 0; e < NEE; ++e) {
    A->lateral[e] = s->lateral[e];
    A->stance[e] = p->d_stance[e];
  }
  A->l_upper = s->l_upper; A->l_lower = s->l_lower;
  const DevPlan &D = p->dp;
  A->T.height = D.height; A->T.hcell = D.hcell; A->T.hx0 = D.hx0; A->T.hy0 = D.hy0;
  A->T.n_maps = D.n_maps; A->T.hnx = D.hnx; A->T.hny = D.hny; A->T.terrain_mode = D.terrain_mode;
  A->capacity = s->capacity; A->first_row = s->first_row; A->n_rows = s->n_rows;
  A->accumulate = (s->flags & QTOS_FIT_ACCUMULATE) != 0;
  return 0;
}

int qtos_force_fit_device(QtosPlanner *p, int B, const QtosForceFit *s, const double *d_nodes, const double *d_t0, const int *d_map_id,
                          const int *d_first_row, const int *d_n_rows, const long long *d_cursor, const double *d_joint,
                          const double *d_mass_scale, double *d_rows, int *d_status, QtosCheckRecord *d_summary, void *stream_) {
  FitArgs A;
  if (force_fit_args(p, B, s, d_nodes, d_t0, d_cursor, d_rows, d_status, d_summary, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_force_fit, dim3(B), dim3(FIT_TILE), 0, (hipStream_t)stream_, p->d_sp, A, d_nodes, d_t0, d_map_id, d_first_row,
                     d_n_rows, d_cursor, d_joint, d_mass_scale, d_rows, d_status, (CheckRecord *)d_summary, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_force_fit(QtosPlanner *p, int B, const QtosForceFit *s, const double *nodes, const double *t0, const int *map_id,
                   const int *first_row, const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale,
                   double *rows, int *status, QtosCheckRecord *summary) {
  FitArgs A;
  if (force_fit_args(p, B, s, nodes, t0, cursor, rows, status, summary, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t nr = segment_elems(B, A.capacity, A.n_rows);
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_map = S.in(map_id, B), *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_joint = S.in(joint, nr * QTOS_CSV_COLS), *d_ms = S.in(mass_scale, B);
  double *d_rows = S.inout(rows, nr * FIT_COLS);                                   // (rows behind a window's count come back as they were)
  int *d_st = S.inout(status, nr);
  QtosCheckRecord *d_sum = S.inout(summary, (size_t)B * FIT_FAMILIES);             // (the accumulate flag merges with what is there)
  if (S.rc) return S.rc;
  const int rc = qtos_force_fit_device(p, B, s, d_nodes, d_t0, d_map, d_first, d_n, d_cur, d_joint, d_ms, d_rows, d_st, d_sum, nullptr);
  return rc ? rc : S.download();
}

// ---- the force fit inside the friction pyramid (k_force_qp, window_kernels.hpp) -----------------------------------
// QtosForceQp begins with QtosForceFit's fields in its order, so the fit's checks and FitArgs are force_fit_args' on that part.
static int force_qp_args(QtosPlanner *p, int B, const QtosForceQp *s, const void *nodes, const void *t0, const void *cursor,
                         const void *rows, const void *qrows, const void *status, const void *summary, FitArgs *A, QpArgs *Q) {
  if (!p) return -1;
  static_assert(offsetof(QtosForceQp, mu) == sizeof(QtosForceFit), "QtosForceQp repeats QtosForceFit's layout");
  QtosForceFit fit;
  if (s) memcpy(&fit, s, sizeof fit);
  const char *why = nullptr;
  if (force_fit_args(p, B, s ? &fit : nullptr, nodes, t0, cursor, rows, status, summary, A)) {
    p->err.replace(0, strlen("qtos_force_fit"), "qtos_force_qp");
    return -1;
  }
  if (qrows && !rows) why = "qrows go with rows";
  else if (!(s->mu > 0) || !(s->mu <= 1.7976931348623157e308)) why = "mu is > 0";
  else if (!(s->f_max > 0) || !(s->f_max <= 1.7976931348623157e308)) why = "f_max is > 0";
  else if (!(s->mu_end > 0) || !(s->mu_end <= 1.7976931348623157e308)) why = "mu_end is > 0";
  else if (s->act_tol != s->act_tol) why = "act_tol is not a number";
  else if (s->max_iter < 1 || s->max_iter > QP_MAX_ITER) why = "max_iter is 1 .. 25";
  if (why) {
    p->err = std::string("qtos_force_qp: ") + why;
    return -1;
  }
  A->mu = s->mu; A->f_max = s->f_max;
  Q->mu = s->mu; Q->f_max = s->f_max; Q->mu_end = s->mu_end; Q->act_tol = s->act_tol; Q->max_iter = s->max_iter;
  return 0;
}

int qtos_force_qp_device(QtosPlanner *p, int B, const QtosForceQp *s, const double *d_nodes, const double *d_t0, const int *d_map_id,
                         const int *d_first_row, const int *d_n_rows, const long long *d_cursor, const double *d_joint,
                         const double *d_mass_scale, double *d_rows, double *d_qrows, int *d_status, QtosCheckRecord *d_summary,
                         void *stream_) {
  FitArgs A;
  QpArgs Q;
  if (force_qp_args(p, B, s, d_nodes, d_t0, d_cursor, d_rows, d_qrows, d_status, d_summary, &A, &Q)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_force_qp, dim3(B), dim3(QP_TILE), 0, (hipStream_t)stream_, p->d_sp, A, Q, d_nodes, d_t0, d_map_id, d_first_row,
                     d_n_rows, d_cursor, d_joint, d_mass_scale, d_rows, d_qrows, d_status, (CheckRecord *)d_summary, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_force_qp(QtosPlanner *p, int B, const QtosForceQp *s, const double *nodes, const double *t0, const int *map_id,
                  const int *first_row, const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale,
                  double *rows, double *qrows, int *status, QtosCheckRecord *summary) {
  FitArgs A;
  QpArgs Q;
  if (force_qp_args(p, B, s, nodes, t0, cursor, rows, qrows, status, summary, &A, &Q)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t nr = segment_elems(B, A.capacity, A.n_rows);
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_map = S.in(map_id, B), *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_joint = S.in(joint, nr * QTOS_CSV_COLS), *d_ms = S.in(mass_scale, B);
  double *d_rows = S.inout(rows, nr * FIT_COLS), *d_qrows = S.inout(qrows, nr * QP_COLS);
  int *d_st = S.inout(status, nr);
  QtosCheckRecord *d_sum = S.inout(summary, (size_t)B * FIT_FAMILIES);
  if (S.rc) return S.rc;
  const int rc = qtos_force_qp_device(p, B, s, d_nodes, d_t0, d_map, d_first, d_n, d_cur, d_joint, d_ms, d_rows, d_qrows, d_st, d_sum, nullptr);
  return rc ? rc : S.download();
}

// ---- the rollout with the force QP in every step (k_rollout_qp, window_kernels.hpp) ------------------------------
// QtosRolloutQp begins with QtosRolloutFeet's fields at its offsets, so the body's and the feet's checks are rollout_feet_args' on
// that part; then the QP's own.
static int rollout_qp_args(QtosPlanner *p, int B, const QtosRolloutQp *s, const void *nodes, const void *t0, const void *cursor,
                           const void *state, const void *count, const void *word, const void *meas, const void *status, RolloutArgs *A,
                           FeetArgs *F, QpArgs *Q) {
  if (!p) return -1;
  static_assert(offsetof(QtosRolloutQp, feet_flags) == offsetof(QtosRolloutFeet, feet_flags) && offsetof(QtosRolloutQp, arm) == offsetof(QtosRolloutFeet, arm) &&
                    offsetof(QtosRolloutQp, f_max) == offsetof(QtosRolloutFeet, f_max) && offsetof(QtosRolloutQp, push_ticks) == offsetof(QtosRolloutFeet, push_ticks),
                "QtosRolloutQp begins with QtosRolloutFeet's fields");
  QtosRolloutFeet feet;
  if (s) {
    std::memcpy(&feet, s, offsetof(QtosRolloutFeet, feet_flags));
    feet.feet_flags = 0;
  }
  if (rollout_feet_args(p, B, s ? &feet : nullptr, nodes, t0, cursor, state, count, word, meas, status, A, F)) {
    p->err = "qtos_rollout_qp: " + p->err.substr(p->err.find(": ") + 2);
    return -1;
  }
  const char *why = nullptr;
  if (!(s->mu > 0) || !(s->mu <= 1.7976931348623157e308)) why = "mu is > 0";
  else if (!(s->f_max > 0) || !(s->f_max <= 1.7976931348623157e308)) why = "f_max is > 0";
  else if (!(s->mu_end > 0) || !(s->mu_end <= 1.7976931348623157e308)) why = "mu_end is > 0";
  else if (s->act_tol != s->act_tol) why = "act_tol is not a number";
  else if (s->max_iter < 1 || s->max_iter > QP_MAX_ITER) why = "max_iter is 1 .. 25";
  if (why) {
    p->err = std::string("qtos_rollout_qp: ") + why;
    return -1;
  }
  Q->mu = s->mu; Q->f_max = s->f_max; Q->mu_end = s->mu_end; Q->act_tol = s->act_tol; Q->max_iter = s->max_iter;
  return 0;
}

int qtos_rollout_qp_device(QtosPlanner *p, int B, const QtosRolloutQp *s, const double *d_nodes, const double *d_t0, const int *d_first_row,
                           const int *d_n_rows, const long long *d_cursor, const double *d_joint, const double *d_mass_scale,
                           const double *d_push, double *d_state, long long *d_count, int *d_word, double *d_meas, double *d_rows,
                           double *d_frows, double *d_qrows, int *d_status, void *stream_) {
  RolloutArgs A;
  FeetArgs F;
  QpArgs Q;
  if (rollout_qp_args(p, B, s, d_nodes, d_t0, d_cursor, d_state, d_count, d_word, d_meas, d_status, &A, &F, &Q)) return -1;
  const long long most = most_rows(A.capacity, A.n_rows, d_n_rows != nullptr);
  if (most < 1) return 0;
  HIPCHK(p, hipSetDevice(p->device));
  if (most > ROLLOUT_TICK)
    hipLaunchKernelGGL(k_rollout_qp<ROLLOUT_TILE>, dim3(B), dim3(ROLLOUT_TILE), 0, (hipStream_t)stream_, p->d_sp, A, F, Q, d_nodes, d_t0,
                       d_first_row, d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_frows,
                       d_qrows, d_status, B);
  else
    hipLaunchKernelGGL(k_rollout_qp<ROLLOUT_TICK>, dim3(B), dim3(ROLLOUT_TICK), 0, (hipStream_t)stream_, p->d_sp, A, F, Q, d_nodes, d_t0,
                       d_first_row, d_n_rows, d_cursor, d_joint, d_mass_scale, d_push, d_state, d_count, d_word, d_meas, d_rows, d_frows,
                       d_qrows, d_status, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_rollout_qp(QtosPlanner *p, int B, const QtosRolloutQp *s, const double *nodes, const double *t0, const int *first_row,
                    const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                    double *state, long long *count, int *word, double *meas, double *rows_out, double *frows, double *qrows, int *status) {
  RolloutArgs A;
  FeetArgs F;
  QpArgs Q;
  if (rollout_qp_args(p, B, s, nodes, t0, cursor, state, count, word, meas, status, &A, &F, &Q)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t rows = segment_elems(B, A.capacity, A.n_rows);
  const size_t mcols = (A.flags & QTOS_ROLLOUT_QUAT) ? 19 : 18;
  Staging S(p);
  const double *d_nodes = S.in(nodes, (size_t)B * p->M.n_vars), *d_t0 = S.in(t0, B);
  const int *d_first = S.in(first_row, B), *d_n = S.in(n_rows, B);
  const long long *d_cur = S.in(cursor, B);
  const double *d_joint = S.in(joint, rows * QTOS_CSV_COLS), *d_ms = S.in(mass_scale, B), *d_push = S.in(push, (size_t)B * 6);
  double *d_state = S.inout(state, (size_t)B * 13);
  long long *d_count = S.inout(count, B);
  int *d_word = S.inout(word, B);
  double *d_meas = S.inout(meas, rows * mcols), *d_rows = S.inout(rows_out, rows * ROLLOUT_COLS), *d_frows = S.inout(frows, rows * FEET_COLS);
  double *d_qrows = S.inout(qrows, rows * QP_COLS);
  int *d_st = S.inout(status, rows);
  if (S.rc) return S.rc;
  const int rc = qtos_rollout_qp_device(p, B, s, d_nodes, d_t0, d_first, d_n, d_cur, d_joint, d_ms, d_push, d_state, d_count, d_word, d_meas,
                                        d_rows, d_frows, d_qrows, d_st, nullptr);
  return rc ? rc : S.download();
}

// ---- goals of receding windows from their global paths (k_path_goal, window_kernels.hpp) ------------------------
// The argument checks of both forms, and QtosPathGoal as k_path_goal reads it.
static int path_goal_args(const QtosPlanner *p, int B, const QtosPathGoal *g, const void *knots, const void *coef, const void *n_pieces,
                          const void *robot_goal, const void *path_id, const void *height_yx, const void *clock, const void *start,
                          const void *goal_out, const void *done, PathGoalArgs *A) {
  if (!p || B < 1 || !g || !knots || !coef || !n_pieces || !clock || !goal_out) return -1;
  if (g->n_paths < 1 || g->max_pieces < 1 || (!path_id && g->n_paths < B)) return -1;
  if (height_yx && (g->n_maps < 1 || g->rows < 1 || g->cols < 1)) return -1;
  if (!(g->cell > 0) || !(g->step_size >= 0)) return -1;
  if (g->base != 0 && g->base != 1) return -1;
  if ((g->clamp_x && !robot_goal) || (g->hold_done && !done)) return -1;
  if (!start && (g->base == 1 || g->stop_dist > 0 || g->hold_done)) return -1;
  A->horizon = g->horizon; A->step_size = g->step_size; A->tol = g->tol; A->z_offset = g->z_offset;
  A->cell = g->cell; A->origin_x = g->origin_x; A->origin_y = g->origin_y;
  A->t_stop = g->t_stop; A->stop_dist = g->stop_dist;
  A->base = g->base; A->clamp_x = g->clamp_x != 0; A->advance_clock = g->advance_clock != 0; A->hold_done = g->hold_done != 0;
  A->n_paths = g->n_paths; A->max_pieces = g->max_pieces;
  A->n_maps = g->n_maps; A->rows = g->rows; A->cols = g->cols;
  return 0;
}

int qtos_path_goal_device(QtosPlanner *p, int B, const QtosPathGoal *g, const double *d_knots, const double *d_coef, const int *d_n_pieces,
                          const double *d_robot_goal, const int *d_path_id, const double *d_height_yx, const int *d_map_id, double *d_clock,
                          const double *d_offset, const double *d_start, double *d_goal_out, int *d_done, void *stream_) {
  PathGoalArgs A;
  if (path_goal_args(p, B, g, d_knots, d_coef, d_n_pieces, d_robot_goal, d_path_id, d_height_yx, d_clock, d_start, d_goal_out, d_done, &A))
    return -1;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_path_goal, dim3((B + 63) / 64), dim3(64), 0, (hipStream_t)stream_, A, d_knots, d_coef, d_n_pieces, d_robot_goal,
                     d_path_id, d_height_yx, d_map_id, d_clock, d_offset, d_start, d_goal_out, d_done, B);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_path_goal(QtosPlanner *p, int B, const QtosPathGoal *g, const double *knots, const double *coef, const int *n_pieces,
                   const double *robot_goal, const int *path_id, const double *height_yx, const int *map_id, double *clock,
                   const double *offset, const double *start, double *goal_out, int *done) {
  PathGoalArgs A;
  if (path_goal_args(p, B, g, knots, coef, n_pieces, robot_goal, path_id, height_yx, clock, start, goal_out, done, &A)) return -1;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t np_ = (size_t)g->n_paths, mp = (size_t)g->max_pieces;
  Staging S(p);
  const double *d_knots = S.in(knots, np_ * (mp + 1)), *d_coef = S.in(coef, np_ * 8 * mp);
  const int *d_n = S.in(n_pieces, np_);
  const double *d_rg = S.in(robot_goal, np_ * 3);
  const int *d_pid = S.in(path_id, B);
  const double *d_h = S.in(height_yx, (size_t)g->n_maps * g->rows * g->cols);
  const int *d_mid = S.in(height_yx ? map_id : nullptr, B);
  double *d_clock = S.inout(clock, B, 0, g->advance_clock != 0);   // (the clock comes back where the kernel advances it)
  const double *d_off = S.in(offset, B), *d_start = S.in(start, (size_t)B * QTOS_START_DOUBLES);
  int *d_done = S.inout(done, B);
  double *d_goal = S.out(goal_out, (size_t)B * 3);
  if (S.rc) return S.rc;
  const int rc = qtos_path_goal_device(p, B, g, d_knots, d_coef, d_n, d_rg, d_pid, d_h, d_mid, d_clock, d_off, d_start, d_goal, d_done, nullptr);
  return rc ? rc : S.download();
}

// ---- the global paths of receding windows (k_path_plan, window_kernels.hpp) --------------------------------------
// The argument checks of both forms, and QtosPathPlan as k_path_plan reads it.  The kernel's LDS is laid out for these limits.
static int path_plan_args(QtosPlanner *p, int B, const QtosPathPlan *g, const void *bool_maps, const void *start, const void *robot_goal,
                          const void *knots, const void *coef, const void *n_pieces, const void *n_cells, const void *status,
                          const void *done, PathPlanArgs *A) {
  if (!p) return -1;
  const char *why = nullptr;
  if (!g || !bool_maps || !start || !robot_goal || !knots || !coef || !n_pieces || !n_cells || !status) why = "a required pointer is null";
  else if (B < 1) why = "B < 1";
  else if (g->rows < 1 || g->cols < 1 || (long long)g->rows * g->cols > PP_GRID) why = "rows, cols >= 1 and rows * cols <= 16384";
  else if (g->max_open < 1 || g->max_open > PP_OPEN) why = "max_open is 1 .. 4096";
  else if (g->max_pieces < 1) why = "max_pieces >= 1";
  else if (g->max_cells < 1 || g->max_cells > PP_GRID || (long long)g->max_cells > 2LL * g->max_pieces)
    why = "max_cells is 1 .. min(2 * max_pieces, 16384)";
  else if (g->n_maps < 1) why = "n_maps >= 1";
  else if (!(g->cell > 0) || !(g->step_size > 0)) why = "cell and step_size are > 0";
  else if (g->height_bound != g->height_bound) why = "height_bound is not a number";
  else if (g->set_done && !done) why = "set_done needs done";
  if (why) {
    p->err = std::string("qtos_path_plan: ") + why;
    return -2;
  }
  A->cell = g->cell; A->origin_x = g->origin_x; A->origin_y = g->origin_y; A->height_bound = g->height_bound; A->step_size = g->step_size;
  A->rows = g->rows; A->cols = g->cols; A->max_cells = g->max_cells; A->max_open = g->max_open; A->max_pieces = g->max_pieces;
  A->n_maps = g->n_maps; A->set_done = g->set_done != 0;
  return 0;
}

int qtos_path_plan_device(QtosPlanner *p, int B, const QtosPathPlan *g, const double *d_bool_maps, const int *d_map_id, const double *d_start,
                          const double *d_robot_goal, double *d_knots, double *d_coef, int *d_n_pieces, int *d_cells, int *d_n_cells,
                          int *d_status, int *d_done, void *stream_) {
  PathPlanArgs A;
  if (const int rc = path_plan_args(p, B, g, d_bool_maps, d_start, d_robot_goal, d_knots, d_coef, d_n_pieces, d_n_cells, d_status, d_done, &A))
    return rc;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_path_plan, dim3(B), dim3(64), 0, (hipStream_t)stream_, A, d_bool_maps, d_map_id, d_start, d_robot_goal, d_knots, d_coef,
                     d_n_pieces, d_cells, d_n_cells, d_status, d_done);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_path_plan(QtosPlanner *p, int B, const QtosPathPlan *g, const double *bool_maps, const int *map_id, const double *start,
                   const double *robot_goal, double *knots, double *coef, int *n_pieces, int *cells, int *n_cells, int *status, int *done) {
  PathPlanArgs A;
  if (const int rc = path_plan_args(p, B, g, bool_maps, start, robot_goal, knots, coef, n_pieces, n_cells, status, done, &A)) return rc;
  HIPCHK(p, hipSetDevice(p->device));
  const size_t mp = (size_t)g->max_pieces, nb = (size_t)B;
  Staging S(p);
  const double *d_maps = S.in(bool_maps, (size_t)g->n_maps * g->rows * g->cols);
  const int *d_mid = S.in(map_id, nb);
  const double *d_start = S.in(start, nb * QTOS_START_DOUBLES), *d_rg = S.in(robot_goal, nb * 3);
  double *d_knots = S.out(knots, nb * (mp + 1)), *d_coef = S.out(coef, nb * 8 * mp);
  int *d_n = S.out(n_pieces, nb), *d_cells = S.out(cells, nb * g->max_cells * 2), *d_nc = S.out(n_cells, nb), *d_st = S.out(status, nb);
  int *d_done = S.inout(done, nb);
  if (S.rc) return S.rc;
  const int rc = qtos_path_plan_device(p, B, g, d_maps, d_mid, d_start, d_rg, d_knots, d_coef, d_n, d_cells, d_nc, d_st, d_done, nullptr);
  return rc ? rc : S.download();
}

// ---- the probe and the stamp of the windows' heightfields (k_probe*, window_kernels.hpp) -------------------------
// The argument checks of all four forms, and QtosProbe as the kernels read it.  k_probe's LDS is sized from these limits, and
// k_probe_scan's index arithmetic stays within an int for PROBE_MAPS maps.
static constexpr int PROBE_MAPS = 1 << 24;
static int probe_args(QtosPlanner *p, const QtosProbe *g, const char *who, bool pointers, int capacity, ProbeArgs *A) {
  if (!p) return -1;
  const char *why = nullptr;
  if (!g || !pointers) why = "a required pointer is null";
  else if (g->rows < 1 || g->cols < 2 || (long long)g->rows * g->cols > PP_GRID) why = "rows >= 1, cols >= 2 and rows * cols <= 16384";
  else if (g->n_maps < 1 || g->n_maps > PROBE_MAPS) why = "n_maps is 1 .. 16777216";
  else if ((long long)g->n_maps * g->rows * (g->cols / 2 - 1) > 2147483647LL) why = "the slots, n_maps * rows * (cols / 2 - 1), fit an int";
  else if (g->scale < 1 || g->scale > 4) why = "scale is 1 .. 4";
  else if (g->multi_map_shift < 1) why = "multi_map_shift >= 1";
  else if (!(g->cell > 0)) why = "cell is > 0";
  else if (g->origin_shift != g->origin_shift || g->z_offset != g->z_offset) why = "origin_shift or z_offset is not a number";
  else if (capacity < 0) why = "capacity >= 0";
  if (!why)
    for (int e = 0; e < QTOS_NEE; ++e)
      for (int k = 0; k < 3; ++k)
        if (g->nominal_stance[e][k] != g->nominal_stance[e][k]) why = "nominal_stance is not a number";
  if (why) {
    p->err = std::string(who) + ": " + why;
    return -2;
  }
  A->cell = g->cell; A->origin_shift = g->origin_shift; A->z_offset = g->z_offset;
  for (int e = 0; e < QTOS_NEE; ++e)
    for (int k = 0; k < 3; ++k) A->stance[3 * e + k] = g->nominal_stance[e][k];
  A->rows = g->rows; A->cols = g->cols; A->n_maps = g->n_maps; A->scale = g->scale; A->multi_map_shift = g->multi_map_shift;
  A->capacity = capacity;
  return 0;
}

int qtos_probe_device(QtosPlanner *p, const QtosProbe *g, const double *d_map_yx, int capacity, int *d_offsets, int *d_slot, int *d_patch,
                      double *d_start, double *d_goal, int *d_map_id, void *stream_) {
  ProbeArgs A;
  if (const int rc = probe_args(p, g, "qtos_probe", d_map_yx && d_offsets && d_slot && d_patch, capacity, &A)) return rc;
  HIPCHK(p, hipSetDevice(p->device));
  hipStream_t s = (hipStream_t)stream_;
  hipLaunchKernelGGL(k_probe_count, dim3(A.n_maps), dim3(64), 0, s, A, d_map_yx, d_offsets);
  hipLaunchKernelGGL(k_probe_scan, dim3(1), dim3(256), 0, s, d_offsets, A.n_maps);
  hipLaunchKernelGGL(k_probe, dim3(A.n_maps), dim3(64), probe_lds_bytes(A.rows, A.cols), s, A, d_map_yx, d_offsets, d_slot, d_patch, d_start, d_goal, d_map_id);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_probe_stamp_device(QtosPlanner *p, const QtosProbe *g, const int *d_offsets, const int *d_slot, const int *d_patch,
                            const int *d_status, double *d_bool_maps, void *stream_) {
  ProbeArgs A;
  (void)d_patch;                                           // (not read: the kernel finds the patches through slot)
  if (const int rc = probe_args(p, g, "qtos_probe_stamp", d_offsets && d_slot && d_status && d_bool_maps, 0, &A)) return rc;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_probe_stamp, dim3(A.n_maps), dim3(64), 0, (hipStream_t)stream_, A, d_offsets, d_slot, d_status, d_bool_maps);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_probe(QtosPlanner *p, const QtosProbe *g, const double *map_yx, int capacity, int *offsets, int *slot, int *patch, double *start,
               double *goal, int *map_id) {
  ProbeArgs A;
  if (const int rc = probe_args(p, g, "qtos_probe", map_yx && offsets && slot && patch, capacity, &A)) return rc;
  HIPCHK(p, hipSetDevice(p->device));
  // The per-problem outputs are copied in first: what the kernels do not write -- problems beyond N -- comes back as it was.
  // They and slot get an element of pad: no candidate slots (cols < 4) or capacity = 0 leave the kernels a pointer still.
  const size_t cells = (size_t)g->n_maps * g->rows * g->cols, slots = (size_t)g->n_maps * g->rows * (g->cols / 2 - 1), cap = (size_t)capacity;
  Staging S(p);
  const double *d_map = S.in(map_yx, cells);
  int *d_off = S.out(offsets, (size_t)g->n_maps + 1), *d_slot = S.out(slot, slots, 1), *d_patch = S.inout(patch, cap * 3, 1);
  double *d_start = S.inout(start, cap * QTOS_START_DOUBLES, 1), *d_goal = S.inout(goal, cap * 3, 1);
  int *d_mid = S.inout(map_id, cap, 1);
  if (S.rc) return S.rc;
  const int rc = qtos_probe_device(p, g, d_map, capacity, d_off, d_slot, d_patch, d_start, d_goal, d_mid, nullptr);
  return rc ? rc : S.download();
}

int qtos_probe_stamp(QtosPlanner *p, const QtosProbe *g, const int *offsets, const int *slot, const int *patch, const int *status,
                     double *bool_maps) {
  ProbeArgs A;
  (void)patch;                                             // (not read: the kernel finds the patches through slot)
  if (const int rc = probe_args(p, g, "qtos_probe_stamp", offsets && slot && status && bool_maps, 0, &A)) return rc;
  if (offsets[g->n_maps] < 0) {
    p->err = "qtos_probe_stamp: offsets[n_maps] < 0";
    return -2;
  }
  HIPCHK(p, hipSetDevice(p->device));
  const size_t cells = (size_t)g->n_maps * g->rows * g->cols, slots = (size_t)g->n_maps * g->rows * (g->cols / 2 - 1), N = (size_t)offsets[g->n_maps];
  Staging S(p);
  const int *d_off = S.in(offsets, (size_t)g->n_maps + 1);
  const int *d_slot = S.in(slot, slots, 1), *d_status = S.in(status, N, 1);   // (an element of pad: an empty array is a pointer still)
  double *d_bm = S.out(bool_maps, cells);
  if (S.rc) return S.rc;
  const int rc = qtos_probe_stamp_device(p, g, d_off, d_slot, nullptr, d_status, d_bm, nullptr);
  return rc ? rc : S.download();
}

// ---- the randomised terrain of the windows (k_terrain_env, window_kernels.hpp) -----------------------------------
static constexpr int ENV_CELLS = 1 << 24, ENV_SHIFTS = 1 << 20, ENV_PASSES = 1 << 10;
static int terrain_env_args(QtosPlanner *p, const QtosTerrainEnv *g, const double *base, const int *base_id, const unsigned long long *seed,
                            const int *draws, const double *map_yx, const double *height_xy, const int *status, TerrainEnvArgs *A) {
  if (!p) return -1;
  const char *why = nullptr;
  if (!g || !base || !seed || !map_yx || !status) why = "a required pointer is null";
  else if (g->n_maps < 1 || g->n_maps > PROBE_MAPS) why = "n_maps is 1 .. 16777216";
  else if (g->n_base < 1) why = "n_base >= 1";
  else if (!base_id && g->n_base < g->n_maps) why = "without base_id map m reads base m: n_base >= n_maps";
  else if (g->rows < 1 || g->cols < 1 || (long long)g->rows * g->cols > ENV_CELLS) why = "rows >= 1, cols >= 1 and rows * cols <= 16777216";
  else if (g->n_shift < 0 || g->n_shift > ENV_SHIFTS) why = "n_shift is 0 .. 1048576";
  else if (g->n_height < 0 || g->n_height > ENV_PASSES) why = "n_height is 0 .. 1024";
  else if (!(g->delta >= 0) || !(g->delta <= 1.7976931348623157e308)) why = "delta is a finite number >= 0";
  if (!why) {                                              // the workgroups read and write side by side: no output may lie over another array
    const size_t n = (size_t)g->n_maps, grid = n * g->rows * g->cols * sizeof(double);
    struct Span { const char *lo; size_t bytes; bool out; };
    const Span spans[] = {
        {(const char *)base, (size_t)g->n_base * g->rows * g->cols * sizeof(double), false}, {(const char *)base_id, n * sizeof(int), false},
        {(const char *)seed, n * sizeof(unsigned long long), false}, {(const char *)draws, n * sizeof(int), true},
        {(const char *)map_yx, grid, true}, {(const char *)height_xy, grid, true}, {(const char *)status, n * sizeof(int), true}};
    for (const Span &a : spans)
      for (const Span &b : spans)
        if (&a < &b && (a.out || b.out) && a.lo && b.lo && a.lo < b.lo + b.bytes && b.lo < a.lo + a.bytes)
          why = "an output (draws, map_yx, height_xy, status) overlaps another array of the call";
  }
  if (why) {
    p->err = std::string("qtos_terrain_env: ") + why;
    return -2;
  }
  A->delta = g->delta;
  A->n_maps = g->n_maps; A->n_base = g->n_base; A->rows = g->rows; A->cols = g->cols;
  A->n_shift = g->n_shift; A->n_height = g->n_height; A->climb = g->climb != 0;
  return 0;
}

int qtos_terrain_env_device(QtosPlanner *p, const QtosTerrainEnv *g, const double *d_base_yx, const int *d_base_id,
                            const unsigned long long *d_seed, int *d_draws, double *d_map_yx, double *d_height_xy, int *d_status,
                            void *stream_) {
  TerrainEnvArgs A;
  if (const int rc = terrain_env_args(p, g, d_base_yx, d_base_id, d_seed, d_draws, d_map_yx, d_height_xy, d_status, &A)) return rc;
  HIPCHK(p, hipSetDevice(p->device));
  hipLaunchKernelGGL(k_terrain_env, dim3(A.n_maps), dim3(ENV_T), 0, (hipStream_t)stream_, A, d_base_yx, d_base_id, d_seed, d_draws, d_map_yx,
                     d_height_xy, d_status);
  HIPCHK(p, hipGetLastError());
  return 0;
}

int qtos_terrain_env(QtosPlanner *p, const QtosTerrainEnv *g, const double *base_yx, const int *base_id, const unsigned long long *seed,
                     int *draws, double *map_yx, double *height_xy, int *status) {
  TerrainEnvArgs A;
  if (const int rc = terrain_env_args(p, g, base_yx, base_id, seed, draws, map_yx, height_xy, status, &A)) return rc;
  if (base_id)
    for (int m = 0; m < g->n_maps; ++m)
      if (base_id[m] < 0 || base_id[m] >= g->n_base) {
        p->err = "qtos_terrain_env: base_id is 0 .. n_base - 1";
        return -2;
      }
  HIPCHK(p, hipSetDevice(p->device));
  // The outputs are copied in first: a map with a non-zero status comes back as it was.
  const size_t cells = (size_t)g->rows * g->cols, n = (size_t)g->n_maps;
  Staging S(p);
  const double *d_base = S.in(base_yx, (size_t)g->n_base * cells);
  const int *d_bid = S.in(base_id, n);
  const unsigned long long *d_seed = S.in(seed, n);
  int *d_draws = S.inout(draws, n), *d_status = S.inout(status, n);
  double *d_map = S.inout(map_yx, n * cells), *d_hxy = S.inout(height_xy, n * cells);
  if (S.rc) return S.rc;
  const int rc = qtos_terrain_env_device(p, g, d_base, d_bid, d_seed, d_draws, d_map, d_hxy, d_status, nullptr);
  return rc ? rc : S.download();
}
