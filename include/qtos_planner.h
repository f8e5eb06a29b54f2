/*
 * qtos_planner.h -- C ABI of the MI355X-native batched local planner.
 *
 * Drop-in boundary.  In the reference the local planner is a process:
 *     subprocess.run("docker exec <id> ./main " + cmd_args(args))
 *         scripts/main.py:49-50, 90-91, 125-126; scripts/run.py:294-295;
 *         QTOS/generateHeightField.py:385-386   (one NLP per call, 32 callers at once)
 * with the flag set of QTOS/utils.py:26 (_flags), the terrain pushed beforehand as a text file
 * (QTOS/utils.py:21-22) and the result fetched as build/traj.csv (QTOS/utils.py:16,19).
 * Every entry point below names the piece of that process ABI it replaces.  Plain pointers and
 * sizes only; no C++ or torch types; no global state; one planner handle is used by one thread
 * at a time (use one handle per (device, stream)).
 *
 * All floating point is IEEE double (the reference solver is double precision throughout).
 */
#ifndef QTOS_PLANNER_H
#define QTOS_PLANNER_H

#ifdef __cplusplus
extern "C" {
#endif

#define QTOS_NEE 4
#define QTOS_MAX_PHASES 32
#define QTOS_START_DOUBLES 24 /* CoM 3, Euler 3, feet FL FR HL HR 12, lin vel 3, Euler rates 3 */
#define QTOS_CSV_COLS 37

/* Model + transcription + solver parameters.  Replaces the constants compiled into the
 * reference's ./main (towr Parameters / RobotModel of the towr_solo12 fork; values recovered from
 * the committed artefacts) and the Ipopt options. */
typedef struct QtosParams {
  int n_phases[QTOS_NEE];                       /* odd: stance, swing, ..., stance            */
  double phase_dur[QTOS_NEE][QTOS_MAX_PHASES];  /* [s]; each foot sums to the plan duration   */
  double dt_base, dt_dyn, dt_rom;               /* base poly / dynamics / range-of-motion dt  */
  int force_polys_per_stance;
  double mass, gravity, inertia_b[9];
  double nominal_stance[QTOS_NEE][3], max_dev[3];
  double mu, f_max, t_swing_avg;
  int honor_start_velocity; /* 0 = reference behaviour (plans start at rest), 1 = use s_vel */
  int terrain_mode;         /* 0 bilinear heightfield (exact slope), 1 nearest cell (flat ledges) */
  int max_iter;
  double tol, mu_init, mu_min, delta_x, eps_dual;
  double slack_push; /* cold-start slack push, fraction of the bound range (0.2) */
  double warm_slack_push; /* the same for a solve that is given `warm` nodes (or a table guess): Ipopt's 0.01 keeps a
                             feasible warm start where it is; a time-shifted previous plan is only a guess and
                             does better with a larger push; 0 = 0.01 */
  int stall_iters;   /* stop a problem (status 1, best iterate returned) after this many iterations
                        without a new lowest violation; 0 = only the iteration limit stops it */
  int hold_from;     /* two-phase solve: once an iterate (number >= hold_from) has brought the constraint
                        violation down to hold_tol, the stance footholds stay where they are (their x, y
                        get the proximal weight hold_weight instead of delta_x): the first iterations
                        place the feet, the rest of the solve is a fixed-foothold problem; 0 = never */
  double hold_weight, hold_tol;
  double chord_tol;  /* an iterate with violation <= chord_tol that was reached by a full step (alpha = 1) of a
                        freshly factored KKT system is followed by a chord step: the stored factorisation is
                        reused with the right-hand side of the new iterate (k_chord: forward + backward sweep over
                        the factor panels, about a fifth of a factorisation); 0 = every iteration factors */
  int reduce_base;   /* 1: inside the KKT solve the base node values are replaced by the coefficients of a clamped cubic
                        B-spline on the same knots (a basis of the C2 splines the acceleration-continuity rows describe):
                        no multipliers for those rows, half the base unknowns, the same Newton step; 0: every row of the
                        reference's NLP has its multiplier (the formulation the internals' tests pin) */
  int chord_max;     /* chord steps in a row with one factorisation (0 = 1): a further one follows a full chord step that
                        brought the violation down to chord_shrink times what it was (and to chord_tol) -- a solve that a
                        chord step leaves just above the tolerance finishes with a second one instead of a factorisation */
  double chord_shrink; /* (0 = 1/3) */
  double stall_alpha;  /* a problem whose step length stays below stall_alpha for two iterations in a row is jammed against its
                          bounds (it would sit there until a division overflows, and its batch with it): it stops like a
                          stalled one -- status 1, best iterate returned; 0 = never */
  int reduce_swing;    /* 1: the swing rule (towr SwingConstraint: the x, y of a swing's mid node = centre of the neighbouring
                          footholds, its v_x, v_y = their distance / t_swing_avg -- constant coefficients) leaves the KKT system:
                          inside the solve the four mid-node variables of every swing are their linear image of the two footholds
                          (no variables, no multipliers for them: 8 unknowns per swing), exactly as reduce_base treats the base's
                          continuity rows.  The iterate, results and CSV keep the mid nodes.  The rows then hold for every
                          iterate only if they hold for the first: the starting point's mid nodes are placed on the rule
                          (towr's straight-line guess has another v_xy there).  Nearest-cell terrain only (terrain_mode 1);
                          0 = every swing row keeps its multiplier */
  int mu_superlinear;  /* 1: the barrier parameter follows Ipopt's monotone update, mu <- max(tol, mu_min, min(0.2 mu, mu^1.5)) behind a
                          step longer than 0.3 (Ipopt's mu_linear_decrease_factor 0.2 and mu_superlinear_decrease_power 1.5, the
                          defaults the reference's solver runs with; mu^1.5 formed as mu * sqrt(mu)): from mu = 0.02 on the
                          superlinear term is the smaller one.  The floor -- Ipopt's is a tenth of ITS tolerance, 1e-3 in the
                          reference's runs: the same 1e-4 as this planner's tol -- keeps the KKT systems of late iterations
                          as well scaled as those of the fourth (with tol / 10 the GPU <-> oracle gaps of the long horizons
                          doubled).  0: mu <- max(mu_min, 0.2 mu) (rounds 1 - 4) */
  double kappa_sigma;  /* Ipopt's kappa_sigma: behind every step a multiplier is clipped to [mu / (kappa_sigma gap), kappa_sigma mu /
                          gap], at the new gap and the mu of the step (Ipopt's default 1e10: the clip never acts in the product's
                          runs).  Must be > 1 -- there is no "0 = default" here: the field is the struct's last, and an image
                          written for a shorter struct is refused rather than read as a setting */
} QtosParams;

typedef struct QtosDims {
  int n_vars, n_cons;               /* 1040 / 1730 for the reference transcription           */
  int n_free, n_eq, n_ineq;         /* 1005 / 706 / 1024 (logs/towr_log.out:44-52)            */
  int n_ineq_lower, n_ineq_both, n_ineq_upper; /* 112 / 816 / 96                              */
  int n_eq_work;                    /* equality rows after dropping constant/duplicate rows   */
  int n_unknowns;                   /* unknowns of the KKT system the planner solves (with reduce_base: coefficients in place
                                       of base node values); dummy pivots of short stages are NOT counted: arrays by
                                       position have n_stages * pivots entries */
  int n_stages, pivots, front;      /* chain of n_stages fronts, `pivots` eliminated per stage */
  int n_base_nodes, n_dyn_times, n_rom_times, n_rows_csv;
  long long panel_doubles;          /* factor panel storage per problem                       */
  long long g_doubles;              /* Jacobian block storage per problem                     */
  long long kkt_algorithmic_bytes;  /* w*[sum_k (p+c_k)*p + 2M], SURVEY.md 8d formula          */
  long long kkt_flops;              /* 2*sum_k p*(p+c_k)^2                                     */
  long long envelope;               /* skyline size of K in the elimination order             */
  int max_active;                   /* largest front actually populated                       */
  int order_rule;                   /* time keys of the elimination order the analysis kept: 0 = rounds 1 - 5 (full-base systems),
                                       1 = late force nodes, 2 = early coefficients (round 6; csrc/model.hpp
                                       HostModel::order_rule, QTOS_ORDER)                                                     */
  double duration;
} QtosDims;

typedef struct QtosPlanner QtosPlanner;

/* Build the planner for one transcription (symbolic KKT analysis + device workspaces for up to
 * max_batch problems on HIP device `device`).  Replaces starting the `towr` container
 * (QTOS/utils.py:686-692 DockerInfo).  Returns 0, or <0: -1 bad parameters, -2 no HIP device /
 * HIP error, -3 out of memory, -4 front too large for LDS.  Nothing here checks that the elimination
 * order the analysis picked is numerically sound for the transcription: where horizons, phase tables or
 * knot spacings vary, use qtos_planner_create_checked (below). */
int qtos_planner_create(const QtosParams *params, int max_batch, int device, QtosPlanner **out);
void qtos_planner_destroy(QtosPlanner *p);
int qtos_planner_dims(const QtosPlanner *p, QtosDims *dims);
const char *qtos_last_error(const QtosPlanner *p);
/* Host-only structure analysis (no GPU needed): the dimensions a planner built from `params`
 * would have; stage_active (may be NULL) receives the populated front size of each stage. */
int qtos_analyze(const QtosParams *params, QtosDims *dims, int *stage_active, int max_stages);
/* Host-only: the schedule by which the idle waves of the KKT kernels' backward sweep form the slack steps ds = Ji dx
 * (round 4; replaces a pass of the line-search kernel).  Per place of a round (16 places per round; round i runs while
 * the sweep solves stage n_stages - 1 - i): constraint row (-1: empty), entries of the row, smallest / largest position
 * of its columns in elimination order.  Arrays may be NULL.  0, or -4: no schedule for this transcription, -5: the packed
 * copy of the column positions disagrees with the list. */
int qtos_analyze_sweep(const QtosParams *params, int *n_rounds, int *rows, int *entries, int *pos_min, int *pos_max, int max_places);
/* Host-only: the elimination order by position, as qtos_debug_structure reports it for a planner (a solver variable's index,
 * n_sol + row for a multiplier -- n_sol = n_vars without reduce_base --, -1 for a dummy pivot): up to max_positions entries into
 * `order`; returns the number of positions (n_stages * pivots) or < 0.  tests/test_order_stability.py eliminates the KKT matrix
 * in this order with numpy, without pivoting, as the chain of fronts does. */
int qtos_analyze_order(const QtosParams *params, int *order, int max_positions);
/* Host-only (round 6, analysis only -- no kernel follows this order yet): what a TWO-ENDED elimination of this model's KKT matrix
 * would look like -- a chain from t = 0 forward, a chain from t = T backward, the unknowns alive across the split time (the
 * separator) last -- and the LDS a workgroup that runs both chains would need.  out (n_out >= 20 ints):
 *   [0] stages today  [1] front today  [2] split stage  [3] stages of chain L  [4] of chain R  [5] separator unknowns
 *   [6] separator stages  [7] front of L  [8] of R  [9] of the separator  [10] serial steps = max([3], [4]) + [6]
 *   [11] populated peak of L  [12] of R;  LDS bytes: [13] today's kernel, of which [14] panels, [15] record buffers, [16] cells;
 *   [17] two chains with today's layouts  [18] two chains with a lean layout (two panels + the blanked copy, one dynamic-only
 *   record buffer per chain, gather tables from L2)  [19] the limit (160 KB - 256 B).  DESIGN.md section 5. */
int qtos_analyze_two_ended(const QtosParams *params, int *out, int n_out);

/* Terrain side channel.  Replaces `docker cp towr_heightfield.txt <id>:...`
 * (QTOS/utils.py:21-22; scripts/main.py:77-78; QTOS/generateHeightField.py:276-279).
 * n_maps height grids of identical shape, height[map][ix*hny+iy] at x = x0+ix*cell,
 * y = y0+iy*cell (the file's row = x index, column = y index: QTOS/generateHeightField.py:568,
 * 598-605).  n_maps = 0 restores flat ground. */
int qtos_set_heightfields(QtosPlanner *p, int n_maps, const double *height, int hnx, int hny,
                          double cell, double x0, double y0);
/* The same from a grid in device memory (d_height: n_maps x hnx x hny doubles, e.g. height_xy of qtos_terrain_env_device):
 * copied device-to-device into the handle's own buffer by a copy queued on `stream`, no host trip.  The handle's buffer is kept
 * where the number of doubles stays what it was (no allocation, no device-wide wait: the terrain of a moving scene is set per
 * step), and replaced otherwise.  Ordering, in both directions, without the caller naming the handle's streams:
 *   - the copy waits (an event, on the device) for the end of the handle's last call, whichever stream that ran on: its kernels
 *     may still read the buffer that is kept;
 *   - every host-pointer entry point (qtos_plan_batch, qtos_probe, qtos_debug_*, ...) runs on the handle's own stream, and that
 *     stream waits for the copy; qtos_plan_batch_device / qtos_plan_submit on any stream wait for it too.
 * Only other work of the caller's own that reads d_height's source or the result on a third stream is the caller's to order.
 * Returns 0; -1 on a null planner, a null d_height with n_maps > 0, hnx or hny < 1, cell not > 0 (the reason in qtos_last_error;
 * the handle's terrain stays); -5 while a call is open (between qtos_plan_submit and the end of qtos_plan_wait: its kernels read
 * the terrain); -2 HIP error.  n_maps = 0 restores flat ground (synchronous, as qtos_set_heightfields). */
int qtos_set_heightfields_device(QtosPlanner *p, int n_maps, const double *d_height, int hnx, int hny,
                                 double cell, double x0, double y0, void *stream);

/* Optional table of nominal plans for the starting point of cold solves (no reference counterpart: the
 * reference's solver always starts from towr's straight-line guess, and so does this planner
 * unless a table is set).  nodes[(j * ndx + i) * n_vars ..] = a solved plan from the rest start at the
 * origin (nominal stance) to the goal (dx[i], dy[j]); grids strictly increasing.  A solve without
 * `warm` then starts from the bilinear interpolation of the table over its goal displacement,
 * shifted to its own start state, and is treated like a warm start.  ndx = 0 removes the table.
 * Host pointers. */
int qtos_set_init_table(QtosPlanner *p, int ndx, const double *dx, int ndy, const double *dy,
                        const double *nodes);

/* One batched solve = B invocations of `./main -g .. -s .. -s_ang .. -e1..-e4 .. [s_vel ..]
 * [s_ang_vel ..]`.  Host-pointer form: copies in, solves on the GPU, copies out.
 *   start   B x 24   CoM, Euler, feet FL FR HL HR (world), CoM velocity, Euler rates
 *                    (exactly columns 1..24 of a CSV row, QTOS/combiner.py:267-274)
 *   goal    B x 3    -g
 *   map_id  B        heightfield index per problem, NULL = map 0
 *   warm    B x n_vars or NULL: starting nodes (receding-horizon warm start)
 *   nodes_out  B x n_vars  solution in the reference NLP's variable order
 *                          (logs/towr_log.out:99-110)
 *   status_out B   0 = solved (the reference's exit code / "status -> 0"), 1 = iteration limit,
 *                  2 = numerical failure (non-finite inputs; or a non-finite step, nodes_out is
 *                  then the best finite iterate)
 *   iters_out B, viol_out B (max constraint violation), either may be NULL
 * Returns 0 or a negative error code; never throws. */
int qtos_plan_batch(QtosPlanner *p, int B, const double *start, const double *goal,
                    const int *map_id, const double *warm, double *nodes_out, int *status_out,
                    int *iters_out, double *viol_out);

/* Same, all pointers in device memory of the planner's device, work queued on `stream` (a hipStream_t passed
 * as void*, NULL = default stream) -- the asynchronous form of the boundary, in three entry points that replace the
 * reference's pool of `docker exec ./main` workers pulling probes from a queue (QTOS/generateHeightField.py:344-352,
 * 375-377; scripts/main.py:49-50 for the single call):
 *
 *   qtos_plan_submit   queues the initial guess and the LAUNCH PATTERN of the handle -- per launch slot the solve kernels
 *                      its last two calls both needed there (a flat walk or trot batch: factorisation x 3, chord solve,
 *                      every time) -- and returns at once: the whole solve is in the queue, the host is not part of the
 *                      Newton loop (round 6).  The first call of a handle queues its first iteration only.  A problem's
 *                      result is written to the output buffers by the kernel that finishes it -- converged, stalled,
 *                      failed or out of iterations --: there is no export step.  A problem that finds the wrong solve
 *                      kernel in a slot of the pattern sits that launch out and takes its step behind a later one: the
 *                      plans are bit for bit those of the informed loop, whatever was queued.
 *                      (qtos_set_speculation(n > 1), rounds 3 - 5: n "blind" iterations instead -- both solve kernels in
 *                      every slot; switches the pattern off.)
 *   qtos_plan_poll     non-blocking: reads the counts of unfinished problems the iterations sent back; a batch that
 *                      needs more iterations gets them queued one by one (only the kernels with work);
 *                      *done = 1 once the counts say that every problem is finished (the results are then in the
 *                      output buffers: the counts travel behind the kernel that wrote them).
 *   qtos_plan_wait     polls until done.
 *
 * qtos_plan_batch_device = submit + wait: it returns when the last iteration has reported that no problem is left; work
 * queued on `stream` afterwards sees the results, and so does the host after synchronising `stream`.  For a batch whose problems all finish within the blind
 * slots of the pattern the host does nothing between the submit and the end but wait for one word.  One planner handle serves one call at a time (a second submit before the first is done returns -5);
 * handles are independent: several handles on their own streams keep several batches in flight from ONE host thread
 * (qtos_amd.pool.PlannerPool: submit to a free handle, poll the others) -- a batch that waits for its slowest problem
 * then shares the GPU with the next ones.  This is the form bench.py times.
 *
 * Environment.  Read ONCE, by qtos_planner_create / qtos_planner_create_checked (and by the host-only qtos_analyze* calls for themselves), in one place
 * (csrc/env.hpp); the planner keeps what it found and qtos_env() hands it back.  Diagnostics and measured alternatives, the
 * defaults are the measured optimum:
 *   QTOS_KKT=2 | 4 | 6       force the factor + solve kernel: k_kkt2 / k_kkt3 MODE 1 / k_kkt5 (default: k_kkt3 MODE 1 for fronts of up
 *                            to 112 slots, k_kkt2 above; see qtos_kkt_kernel below and DESIGN.md section 5).  3 and 5 (k_kkt3 MODE 0,
 *                            k_kkt4 of rounds 4 - 5) select nothing in any build, experiment builds included: a warning on stderr,
 *                            then the default
 *   QTOS_LANES=n             a call of more problems than the GPU has compute units is cut into up to n (<= 4) contiguous parts,
 *                            each with its own host-driven loop on a stream of the planner; bit-identical plans; default 1
 *                            (measured slower than one lock-step loop at 1024 problems per call)
 *   QTOS_SHORT_STAGES=1 | 0  stage boundaries by dynamic programming: 1 = for every front size even at 2 % more stages, 0 = never;
 *                            unset = for fronts above 128 slots by that rule and for smaller fronts only where a 16-slot group
 *                            comes off the front at NO extra stage (walk 128 -> 112 slots, trot 112 -> 96).
 *                            QTOS_NO_SHORT_STAGES=1 is the older spelling of 0
 *   QTOS_SPEC_PATTERN=0      qtos_plan_submit queues the first iteration only and the host reads the counts in front of every
 *                            further one (default 1: the launch pattern below; qtos_set_pattern_speculation does the same per handle)
 *   QTOS_PLACE=1..4          slot placement rule of the analysis (0 = the measured best: a group that hosts the stage's siblings)
 *   QTOS_ORDER=0 | 1 | 2     time keys of the elimination order: 0 = rounds 1 - 5 (force nodes at their node time, B-spline coefficients
 *                            in the middle of their support), 1 = round 6's order with the late force nodes (csrc/model.hpp
 *                            HostModel::order_rule: the 100-knot walk and the 200-knot transcription fit 96 slots instead of 112),
 *                            2 = rule 1 without the late force nodes (coefficients one polynomial earlier, first-knot guard).
 *                            Unset: on a reduced base rules 2 and 1 are analysed and the smaller front is kept (rule 0 loses up to
 *                            six digits of a KKT solve on short trot horizons and is not in the automatic choice there); full-base
 *                            systems keep rule 0
 *   QTOS_SWEEP_DS=0          k_step forms the slack steps ds = Ji dx + (g - s) itself (default 1: three waves that idle in the
 *                            backward sweep of the KKT kernels form them, block by block behind the stage that solves the
 *                            block's earliest column; bit-identical plans)
 *   QTOS_SPEC_JAC=0          k_step evaluates the first trial point of the line search without its Jacobian and linearises in a
 *                            second pass (default 1: one pass behind a Newton step; bit-identical plans) */
int qtos_plan_batch_device(QtosPlanner *p, int B, const double *d_start, const double *d_goal,
                           const int *d_map_id, const double *d_warm, double *d_nodes_out,
                           int *d_status_out, int *d_iters_out, double *d_viol_out, void *stream);

/* Time-shifted warm start for a receding-horizon replan (the reference re-plans from the
 * row `lookahead` steps ahead in the plan being executed, QTOS/combiner.py:245-296, and restarts the gait
 * schedule with every plan): warm_out[b] = the previous plan nodes_prev[b] read at offset[b] + (node time) for
 * every variable of the new plan whose shifted time still lies inside the previous horizon, towr's
 * straight-line guess of the new problem (start[b] -> goal[b]) beyond it, and the new start / goal in the fixed
 * variables.  Pass warm_out as `warm` of qtos_plan_batch*.  offset in seconds (>= 0). */
int qtos_shift_warm(QtosPlanner *p, int B, const double *nodes_prev, const double *offset,
                    const double *start, const double *goal, const int *map_id, double *warm_out);
int qtos_shift_warm_device(QtosPlanner *p, int B, const double *d_nodes_prev, const double *d_offset,
                           const double *d_start, const double *d_goal, const int *d_map_id,
                           double *d_warm_out, void *stream);

/* 1 kHz sampling of solution nodes into the reference's CSV row layout (37 columns,
 * QTOS/utils.py:107-148; producer build/traj.csv).  rows_out is B x n_rows x 37, row k is at
 * local time k/hz and carries time stamp t0[b] + k/hz.  Host pointers. */
int qtos_sample_csv(QtosPlanner *p, int B, const double *nodes, const double *t0, double hz,
                    int n_rows, double *rows_out);
int qtos_sample_csv_device(QtosPlanner *p, int B, const double *d_nodes, const double *d_t0,
                           double hz, int n_rows, double *d_rows_out, void *stream);

/* Hand-over of a receding-horizon replan: which row of the plan being executed the next plan starts from, and that row's
 * state.  Replaces Combiner._state and legs_in_contact (QTOS/combiner.py:78-92,245-296: read the CSV, go `lookahead` rows
 * ahead, move on row by row until every foot stands on a known terrain height, zero_filter the state) for B windows at
 * once, without a table of rows: one workgroup per window (k_handover) tests the candidate rows k0 .. k0 + n_search,
 * k0 = round(advance * hz), n_search = round(search * hz), row k at plan time k / hz (clamped to the plan's duration as
 * qtos_sample_csv clamps it), and evaluates the first that passes; k0 itself where none passes (the reference's fall-back
 * to the un-shifted row).  The numbers are those of qtos_sample_csv's rows, to the bit. */
typedef struct QtosHandover {
  double advance, search, hz;   /* seconds, seconds, rows per second (hz <= 0: 1000) */
  int rule;                     /* 0 force rule: f_z > 0 for all four feet (columns 27, 30, 33, 36 of the row);
                                   1 height-set rule (Combiner._state): every foot's z (columns 9, 12, 15, 18), at 6 decimals,
                                   is one of `heights`: rint(z * 1e6) == rint(h * 1e6) */
  int n_heights;                /* rule 1: 1 .. 8 */
  double heights[8];
  int zero_filter;              /* 1: QTOS/utils.py zero_filter on start_out (|v| < 1e-4 -> 0) */
  int turn;                     /* 1: turn a window round outside [x_lo, x_hi]: goal_step[b][0] = s |goal_step[b][0]|, s = -1 for
                                   start_out[b][0] > x_hi, +1 for start_out[b][0] < x_lo, else the sign it has; in place */
  double x_lo, x_hi;
} QtosHandover;
/* nodes B x n_vars (the windows' newest plans); start_out B x 24 = columns 1 .. 24 of the hand-over row (`start` of the next
 * qtos_plan_batch*); offset_out B = row / hz (the plan time of the hand-over: `offset` of qtos_shift_warm*, the reference's
 * lookahead / hz added to -t, QTOS/combiner.py:173); row_out B (may be NULL) the row index.  goal_step B x 3 (in / out, may be
 * NULL): the displacement of a window's goal per plan; then goal_out[b][0:2] = start_out[b][0:2] + goal_step[b][0:2]
 * (goal_out B x 3, NULL iff goal_step is NULL; goal_out[b][2] is not touched).
 * Device form: all pointers but `h` in device memory, one kernel queued on `stream`, no handle state is read or written but
 * the sampling tables -- launch pattern, totals and report flag stay, a plan call behind it returns the bits it would have
 * returned without it, and it may be queued while a call is open.  Host form: host pointers, through the handle's staging
 * buffers, synchronous; -5 while a call is open (between qtos_plan_submit and the end of qtos_plan_wait), B <= max_batch.
 * Both: -1 on bad arguments -- a null planner or required pointer, B < 1, goal_step without goal_out or the reverse, a rule
 * other than 0 / 1, rule 1 with n_heights outside 1 .. 8, advance < 0, search < 0, k0 beyond the plan's last row, a search of
 * more than a million rows. */
int qtos_handover(QtosPlanner *p, int B, const QtosHandover *h, const double *nodes, double *goal_step,
                  double *start_out, double *goal_out, double *offset_out, int *row_out);
int qtos_handover_device(QtosPlanner *p, int B, const QtosHandover *h, const double *d_nodes,
                         double *d_goal_step /* in/out, may be NULL */, double *d_start_out,
                         double *d_goal_out /* NULL iff d_goal_step is NULL */,
                         double *d_offset_out, int *d_row_out /* may be NULL */, void *stream);

/* Stitching of receding windows: the rows a window has executed, appended to a ring of CSV rows per window.  Replaces
 * Combiner.combine and _truncate_csv (QTOS/combiner.py:125-135, 298-312: the old plan up to the hand-over row, then the new
 * plan, written to the file the controller reads) for B windows at once.  A window executes a chain of plans P0, P1, ...: plan
 * Pi has the nodes x_i and the time stamp t0_i of its first row, its hand-over row r_i is row_out of qtos_handover*, P(i+1)
 * starts from the state of that row and t0_(i+1) = t0_i + r_i / hz.  Row k of a plan is row k of qtos_sample_csv, to the bit:
 * 37 columns, time stamp t0 + k / hz, splines at min(k / hz, T).  The executed trajectory is the concatenation over i of the
 * rows first_row .. first_row + r_i - 1 of Pi: first_row 0 keeps every row (old[:r] ++ new), first_row 1 is what the reference
 * writes, whose pd.read_csv eats row 0 of both files (old[1:][:r] ++ new[1:]: the old plan's hand-over row stays and the new
 * plan starts at its second row).  Both append r_i rows; only the first row differs.
 * One call appends one plan's segment for every window b (k_stitch, one workgroup per window):
 *   n = n_rows ? n_rows[b] : s->n_rows, clamped to 0 .. capacity
 *   traj[b][(cursor[b] + j) mod capacity][0:37] = row first_row + j of plan b with the time stamp t0[b] + (first_row + j) / hz,
 *                                                 j = 0 .. n - 1; the other cells of the ring are not touched
 *   cursor[b] += n       (a running total, never reduced modulo capacity: min(cursor, capacity) rows of the ring are valid,
 *                         the oldest at row cursor mod capacity once cursor >= capacity)
 *   t0[b] += n / hz      if advance_clock: the clock of the window's next plan. */
typedef struct QtosStitch {
  double hz;           /* rows per second (<= 0: 1000) */
  int first_row;       /* 0 clean, 1 the reference's read_csv behaviour; 0 .. 1000000 */
  int n_rows;          /* count for every window where d_n_rows is NULL (>= 0) */
  int advance_clock;   /* 1: t0[b] += n / hz */
  long long capacity;  /* rows per window in the ring (>= 1) */
} QtosStitch;
/* nodes B x n_vars (the plans the segments are taken from: in a loop, the plans qtos_handover* was given); n_rows B (may be
 * NULL: s->n_rows for every window; in a loop, row_out of qtos_handover*); t0 B (in / out); traj B x capacity x 37 (in / out);
 * cursor B (in / out).
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream` (behind qtos_handover_device on the same
 * stream d_n_rows may be its d_row_out), no handle state is read or written but the sampling tables -- launch pattern, totals
 * and report flag stay, a plan call behind it returns the bits it would have returned without it, and it may be queued while a
 * call is open.  Host form: host pointers, synchronous, through device buffers of its own as qtos_sample_csv (not the handle's
 * staging buffers: no -5); the ring is copied in and the whole ring is copied out, the result is what the device form leaves.
 * Both: -1 on a null planner or required pointer, B < 1, capacity < 1, first_row outside 0 .. 1000000, n_rows < 0 where
 * d_n_rows is NULL; -2 on a HIP error; -3 out of memory. */
int qtos_stitch_device(QtosPlanner *p, int B, const QtosStitch *s, const double *d_nodes, const int *d_n_rows /* may be NULL */,
                       double *d_t0 /* in/out */, double *d_traj /* B x capacity x 37 */, long long *d_cursor /* in/out */, void *stream);
int qtos_stitch(QtosPlanner *p, int B, const QtosStitch *s, const double *nodes, const int *n_rows,
                double *t0, double *traj, long long *cursor);

/* Joint commands of the windows' plans: leg inverse kinematics and the motor law, per CSV row.  Replaces what the reference's
 * consumer does once per 1 kHz tick (scripts/run.py:184-200, QTOS/robot/robot.py control_multi: towr_transform, inverse
 * kinematics per leg, MotorModel.convert_to_torque_ff) for B windows at once (k_joint_rows; the rule: joints.py).  Joint row k
 * of a plan has 37 columns: the time stamp of CSV row k (t0 + k / hz, qtos_sample_csv's to the bit), then for the legs FL, FR,
 * HL, HR and their joints HAA, HFE, KFE the angles q (columns 1 .. 12), the rates qdot (13 .. 24) and the torques (25 .. 36), at
 * the plan time min(k / hz, T) of CSV row k:
 *   p_b = R(euler)^T (foot - com) + (0, 0, ee_shift), R = Rz(yaw) Ry(pitch) Rx(roll); v_b its time derivative from the plan's
 *         CoM velocity, Euler rates and the foot spline's first derivative
 *   r = p_b - hip, h^2 = r_y^2 + r_z^2 - lateral^2, c3 = (r_x^2 + h^2 - l_u^2 - l_l^2) / (2 l_u l_l)
 *   q1 = atan2(r_y h + r_z lateral, r_y lateral - r_z h), q3 = knee_sign acos(clip(c3, -1, 1)),
 *   q2 = atan2(-r_x, h) - atan2(l_l sin q3, l_u + l_l cos q3)
 *   on the fold side, c3 < -1/2, where c3 + 1 and h^2 are small differences: h^2 = (r_y - lateral)(r_y + lateral) + r_z^2 (h = 0
 *         where the h^2 above is < 0) and q3 = knee_sign 2 atan2(sqrt(max(a, 0)), sqrt(max(b, 0))) with rho^2 = r_x^2 + h^2,
 *         a = ((l_u + l_l)^2 - rho^2) / (2 l_u l_l) and b = (rho^2 - (l_u - l_l)^2) / (2 l_u l_l), b = 0 where c3 < -1; q1 and q2 as
 *         above with this h and q3.  The status bits are the comparisons of the c3 and h^2 above on both sides
 *   qdot = J^-1 v_b (closed 3 x 3 solve), tau_ff = -J^T R^T f with f the plan's foot force (0 with flags bit 0)
 *   tau = clip(kp (q - q_mes) + kd (qdot - qd_mes) + tau_ff, -tau_max, tau_max); without q_mes the PD terms are left out,
 *         tau_max <= 0: no clip
 * and a status word: bit e the target of foot e is beyond the leg's reach (c3 > 1: the leg is straight and points at it), bit
 * 4 + e inside its folded length (c3 < -1), bit 8 + e nearer to the hip axis than the lateral offset (h^2 < 0, h taken as 0).  A
 * leg with one of these bits has qdot = 0.  Bit 12 + e (QTOS_JOINT_NONFINITE << e): one of leg e's nine numbers q, qdot, tau_ff
 * (tau_ff as the motor law takes it: 0 with QTOS_JOINT_NO_FF) is not finite -- a non-finite node, or a division by a
 * determinant that is exactly zero.  Non-finite input: the two clips are comparisons that keep a NaN, and a leg whose target p_b
 * has a non-finite component has q = qdot = (NaN, NaN, NaN) (with them tau_ff, and tau where it is formed from them) and
 * bit 12 + e; no finite angle or rate comes out of such a target.  Its bits e, 4 + e and 8 + e are what the three comparisons
 * give (none on a NaN).  A non-finite force alone leaves q and qdot as they are, tau_ff non-finite, and sets bit 12 + e.  The
 * other legs of the row are not touched by it unless they read the same number (the CoM, the Euler angles).
 * One unit in the last place inside full stretch (c3 just below 1) the rule has no bit and qdot = J^-1 v_b is unbounded:
 * |qdot| grows as 1 / sin q3.  That is the rule as it stands; see DESIGN.md section 6.
 * Two addressing modes.  capacity 0 (table): out is B x n_rows x 37, status B x n_rows, and out[b][j] is joint row first + j,
 * j = 0 .. n - 1, with first = d_first_row ? d_first_row[b] : first_row and n = d_n_rows ? d_n_rows[b] : n_rows clamped to
 * 0 .. n_rows; rows behind n are not touched.  With n_rows = 1, d_first_row and the measured state that is the 1 kHz tick of B
 * robots in one launch.  capacity > 0 (ring): out is B x capacity x 37, status B x capacity, and joint row first + j goes to ring
 * row (cursor[b] + j) mod capacity, n clamped to 0 .. capacity: qtos_stitch's addressing, but cursor and t0 are only read -- queued
 * in front of qtos_stitch_device on the same stream with the same nodes, n_rows, t0 and cursor, it fills a joint ring row for
 * row with the CSV ring. */
#define QTOS_JOINT_NO_FF 1      /* flags: leave the feed-forward torque out (MotorModel.convert_to_torque) */
#define QTOS_JOINT_NONFINITE 4096 /* status: leg 0's bit "a number of this leg is not finite"; leg e: << e (bits 12 .. 15) */
typedef struct QtosJointRows {
  double hz;                    /* rows per second (<= 0: 1000) */
  int first_row;                /* first row where d_first_row is NULL; 0 .. 1000000 */
  int n_rows;                   /* table mode: rows per window in `out`; both modes: the count where d_n_rows is NULL (>= 0) */
  long long capacity;           /* 0: table mode; > 0: rows per window in the ring */
  double ee_shift;              /* towr_transform's lift of the feet in the base frame */
  double hip[4][3];             /* HAA origins in the base frame */
  double lateral[4];            /* y offset of the foot from the HAA axis in the hip frame */
  double l_upper, l_lower;      /* link lengths (> 0) */
  double knee_sign[4];          /* branch of the knee: -1 / +1 */
  double kp[12], kd[12];        /* per joint (MotorModel.UPDATE_GAIT) */
  double tau_max;               /* <= 0: no clip */
  int flags;                    /* QTOS_JOINT_* */
} QtosJointRows;
/* nodes B x n_vars, t0 B; first_row B, n_rows B, q_mes and qd_mes B x 12 (both or neither) may be NULL; cursor B, NULL in table
 * mode; out and status as above.
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream`, no handle state is read or written but the
 * sampling tables -- it may be queued while a call is open.  Host form: host pointers, synchronous, through device buffers of
 * its own as qtos_stitch (no -5); out and status are copied in and out whole.
 * Both: -1 on a null planner or required pointer, B < 1, capacity < 0, a ring without cursor, a table with n_rows < 1, n_rows < 0,
 * first_row outside 0 .. 1000000, q_mes without qd_mes or the reverse, a link length <= 0; -2 on a HIP error. */
int qtos_joint_rows_device(QtosPlanner *p, int B, const QtosJointRows *s, const double *d_nodes, const double *d_t0,
                           const int *d_first_row /* may be NULL */, const int *d_n_rows /* may be NULL */,
                           const long long *d_cursor /* NULL in table mode */, const double *d_q_mes /* may be NULL */,
                           const double *d_qd_mes /* NULL iff d_q_mes is NULL */, double *d_out, int *d_status, void *stream);
int qtos_joint_rows(QtosPlanner *p, int B, const QtosJointRows *s, const double *nodes, const double *t0, const int *first_row,
                    const int *n_rows, const long long *cursor, const double *q_mes, const double *qd_mes, double *out, int *status);

/* Measured states and tracking errors of the windows: what comes back from the robot, per CSV row.  The counterpart of
 * qtos_joint_rows: replaces what the reference does with the measured state once per 1 kHz tick (scripts/run.py:244-273,
 * QTOS/robot/robot.py traj_vec, QTOS/tracking.py Tracking.update / _update, the test global_COM_xyz[0] >= goal[0]) for B windows
 * at once (k_track, one workgroup per window; the rule: tracking.py).  Track row k of a plan has 26 columns:
 *   0         the time stamp of CSV row k (t0 + k / hz, qtos_sample_csv's to the bit)
 *   1 .. 18   the reference's traj_vec of the measured state: CoM, Euler angles (roll, pitch, yaw), the feet FL, FR, HL, HR in the
 *             world, foot e = com + R (fk_e(q_e) - (0, 0, ee_shift)), fk_e the closed-form chain of the SOLO12 leg (hip + Rx(q1)
 *             (x, lateral, -h), x = -l_u sin q2 - l_l sin(q2 + q3), h = l_u cos q2 + l_l cos(q2 + q3)): the inverse of
 *             towr_transform's lift.  ee_shift 0.015: a robot exactly on its commanded angles and planned pose has zero foot
 *             error; ee_shift 0: the URDF's FOOT link, what the reference's simulator returns
 *   19 .. 23  |plan - measured| of the CoM and of the four feet, against the plan's own row k (qtos_sample_csv's columns 1 .. 3 and
 *             7 .. 18), each sqrt((d0 d0 + d1 d1) + d2 d2)
 *   24, 25    total_com and total_feet after this row
 * meas row: base position (3), Euler angles (3), q of the twelve joints (18 doubles); with QTOS_TRACK_QUAT position, quaternion
 * (x, y, z, w), q (19 doubles): the quaternion is divided by its norm, R formed from it, roll = atan2(R21, R22), pitch =
 * asin(clip(-R20, -1, 1)), yaw = atan2(R10, R00).
 * Per window b, count[b] = (calls, recorded) and total[b] = (total_com, total_feet) are read and written: row j of the call is
 * call c = calls + j + 1; it is recorded iff c >= delay and c != delay + 1 (Tracking.update's branches as they stand: with the
 * reference's delay 500 calls 500, 502, 503, ...), with QTOS_TRACK_CLEAN_DELAY iff c > delay.  A recorded row adds its CoM error
 * to total_com and its four foot errors, FL first, to total_feet, in row order (float64, Tracking._update's order), and counts
 * in `recorded`; then calls += n.  Unrecorded rows carry their pose and errors and repeat the standing totals.
 * Status word of a row: bit 0 recorded, bit 1 measured CoM x >= goal_x[b] (never without goal_x), bit 2 the pitch clip acted
 * (|R20| >= 1, quaternion mode).
 * Non-finite input: nothing is replaced.  A measured row with a non-finite number has non-finite columns wherever that number
 * enters -- the pitch clip is a comparison that keeps a NaN, so a quaternion that is zero, NaN or infinite gives NaN Euler
 * columns and feet, without bit 2 -- and, if the row is recorded, total_com and / or total_feet are non-finite from that row on,
 * in this call and in every later call that takes them in.  Bit 1 is a comparison (false on a NaN).
 * Addressing: qtos_joint_rows' exactly, for `out`, `status` and `meas` alike -- capacity 0: tables of n_rows rows per window,
 * row first + j at [b][j], n = d_n_rows ? d_n_rows[b] : n_rows clamped to 0 .. n_rows, rows behind n untouched, a window with
 * n = 0 keeps its count and total; capacity > 0: rings, row first + j at ring row (cursor[b] + j) mod capacity; cursor and t0 are
 * only read, so it is queued next to qtos_joint_rows_device in front of qtos_stitch_device with the same nodes, t0, n_rows and
 * cursor.  With n_rows = 1 and d_first_row: the tick of B robots. */
#define QTOS_TRACK_QUAT 1          /* flags: meas rows carry a quaternion (19 doubles) */
#define QTOS_TRACK_CLEAN_DELAY 2   /* flags: recorded iff call > delay */
#define QTOS_TRACK_COLS 26
typedef struct QtosTrack {
  double hz;                    /* rows per second (<= 0: 1000) */
  int first_row;                /* first row where d_first_row is NULL; 0 .. 1000000 */
  int n_rows;                   /* table mode: rows per window; both modes: the count where d_n_rows is NULL (>= 0) */
  long long capacity;           /* 0: table mode; > 0: rows per window in the rings */
  double ee_shift;              /* towr_transform's lift, taken off the chain's foot */
  double hip[4][3];             /* HAA origins in the base frame */
  double lateral[4];            /* y offset of the foot from the HAA axis in the hip frame */
  double l_upper, l_lower;      /* link lengths (> 0) */
  int delay;                    /* in calls (>= 0); the reference: 500 */
  int flags;                    /* QTOS_TRACK_* */
} QtosTrack;
/* nodes B x n_vars, t0 B; first_row B and n_rows B may be NULL; cursor B, NULL in table mode; meas B x rows x 18 (19 with
 * QTOS_TRACK_QUAT), rows = n_rows or capacity; goal_x B, may be NULL; count B x 2 and total B x 2 in / out; out B x rows x 26,
 * status B x rows.
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream`, no handle state is read or written but the
 * sampling tables -- it may be queued while a call is open.  Host form: host pointers, synchronous, through device buffers of
 * its own as qtos_joint_rows (no -5); out and status are copied in and out whole.
 * Both: -1 on a null planner or required pointer, B < 1, capacity < 0, a ring without cursor, a table with n_rows < 1, n_rows < 0,
 * first_row outside 0 .. 1000000, delay < 0, a link length <= 0; -2 on a HIP error. */
int qtos_track_device(QtosPlanner *p, int B, const QtosTrack *s, const double *d_nodes, const double *d_t0,
                      const int *d_first_row /* may be NULL */, const int *d_n_rows /* may be NULL */,
                      const long long *d_cursor /* NULL in table mode */, const double *d_meas, const double *d_goal_x /* may be NULL */,
                      long long *d_count /* in/out */, double *d_total /* in/out */, double *d_out, int *d_status, void *stream);
int qtos_track(QtosPlanner *p, int B, const QtosTrack *s, const double *nodes, const double *t0, const int *first_row,
               const int *n_rows, const long long *cursor, const double *meas, const double *goal_x, long long *count, double *total,
               double *out, int *status);

/* Feedback hand-over: the next plan starts from where the robot is.  qtos_handover* starts every new plan from the old plan's
 * own hand-over row (the reference's Combiner._state; it records robot_state in Global_Planner.update and never uses it); this
 * call corrects that start vector, in place, by the tracking error of the plan handed over from, for B windows in one launch
 * (k_start_feedback, one lane per window; the rule: feedback.py).  With every gain 0 it changes nothing, to the bit: steps 6
 * and 7 are left out, the status word has bits 1 and 2 only.  Per window b, with r = row[b] the hand-over row (qtos_handover's
 * row_out) and lat = round(latency * hz):
 *   1  the measured plan row is k = clamp(r - lat, first_row, first_row + r - 1), one of the rows qtos_stitch appends for this
 *      plan; its measurement is meas[b][k - first_row] (capacity 0: a B x n_rows x cols table) or ring row (cursor[b] + k -
 *      first_row) mod capacity (qtos_track's addressing), cols 18, or 19 with QTOS_FEEDBACK_QUAT.  r <= 0, or a row the table or
 *      ring does not hold (k - first_row >= n_rows or capacity): status bit 5, and nothing else of the window is touched
 *   2  m[0 .. 17], the measured pose: qtos_track's columns 1 .. 18 of that row, to the bit (status bit 2: the pitch clip acted)
 *   3  p[0 .. 17], the planned pose: qtos_sample_csv's columns 1 .. 18 of plan row k, to the bit
 *   4  e = m - p, the yaw component through the IEEE remainder with 2 pi, every component clipped to +- max_pos (CoM), +- max_ang
 *      (Euler), +- max_foot (feet); status bit 1: a clip acted.  err_out[b] = the clipped e
 *   5  start[0 .. 2] += gain_pos e[0 .. 2], start[3 .. 5] += gain_ang e[3 .. 5], start[6 + 3 f + i] += gain_foot e[6 + 3 f + i]
 *      (a gain of 0 adds nothing: the bits stay).  The velocities, start[18 .. 23], stay the plan's
 *   6  QTOS_FEEDBACK_SNAP: every foot's z becomes the terrain height under its corrected x, y, from the handle's heightfield
 *      map_id[b] in the handle's terrain_mode (the solver's own lookup) -- the first stance fixes the foot where the start vector
 *      puts it, and the terrain row of its second node demands z = h(x, y); status bit 6 + f: that moved foot f's z by more
 *      than snap_tol against the corrected z
 *   7  range-of-motion guard: with R of the corrected Euler angles, d_f = R^T (foot_f - com) - nominal[f]; unless every |d_f[i]|
 *      <= max_deviation[i] + rom_tol (a NaN fails) the window falls back: its start is not written, status bit 3
 *   8  status bit 0: corrected (a measurement, a gain that is not 0, no fallback).  QTOS_FEEDBACK_ZERO_FILTER: |v| < 1e-4 -> 0 on
 *      the 24 doubles of a window that did not fall back (QtosHandover.zero_filter).  With goal_step: goal[b][0 .. 1] =
 *      start[b][0 .. 1] + goal_step[b][0 .. 1] from the start as it stands then; goal[b][2] is not touched */
#define QTOS_FEEDBACK_QUAT 1         /* meas rows carry a quaternion (19 doubles), as QTOS_TRACK_QUAT */
#define QTOS_FEEDBACK_SNAP 2
#define QTOS_FEEDBACK_ZERO_FILTER 4
typedef struct QtosFeedback {
  double hz;                    /* rows per second (<= 0: 1000) */
  int first_row, n_rows;        /* first row of the segment, 0 .. 1000000; table mode: rows per window (>= 1) */
  long long capacity;           /* 0: table mode; > 0: rows per window in the ring */
  double latency;               /* seconds (>= 0): the measurement is that much older than the hand-over row */
  double ee_shift;              /* the leg chain, as QtosTrack */
  double hip[4][3];
  double lateral[4];
  double l_upper, l_lower;      /* link lengths (> 0) */
  double gain_pos, gain_ang, gain_foot;   /* each in 0 .. 1 */
  double max_pos, max_ang, max_foot;      /* clips (> 0) */
  double nominal[4][3];         /* the range-of-motion box of the planner's model: nominal stance ... */
  double max_deviation[3];      /* ... and half widths */
  double rom_tol, snap_tol;
  int flags;                    /* QTOS_FEEDBACK_* */
} QtosFeedback;
/* nodes B x n_vars and t0 B: the plan handed over from and its clock, as qtos_track takes them (in front of qtos_stitch); row B;
 * cursor B, NULL in table mode; meas B x rows x 18 (19 with QTOS_FEEDBACK_QUAT), rows = n_rows or capacity; map_id B, may be
 * NULL: map 0; start B x 24 in / out; goal_step B x 3 and goal B x 3, both or neither; err_out B x 18, may be NULL; status B.
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream`; no handle state is read or written but the
 * sampling tables, the heightfields and their geometry -- it may be queued while a call is open.  Host form: host pointers,
 * synchronous, through device buffers of its own as qtos_track (no -5).
 * Both: -1 on a null planner or required pointer, B < 1, capacity < 0, a ring without cursor, a table with n_rows < 1, first_row
 * outside 0 .. 1000000, latency < 0, a gain outside 0 .. 1, a clip <= 0, a link length <= 0, goal_step without goal or the
 * reverse; -2 on a HIP error; -3 out of memory. */
int qtos_start_feedback_device(QtosPlanner *p, int B, const QtosFeedback *s, const double *d_nodes, const double *d_t0, const int *d_row,
                               const long long *d_cursor /* NULL in table mode */, const double *d_meas,
                               const int *d_map_id /* may be NULL: map 0 */, double *d_start /* in/out, B x 24 */,
                               const double *d_goal_step /* may be NULL */, double *d_goal /* NULL iff d_goal_step is NULL */,
                               double *d_err_out /* B x 18, may be NULL */, int *d_status, void *stream);
int qtos_start_feedback(QtosPlanner *p, int B, const QtosFeedback *s, const double *nodes, const double *t0, const int *row,
                        const long long *cursor, const double *meas, const int *map_id, double *start, const double *goal_step,
                        double *goal, double *err_out, int *status);

/* Plan check: what a plan violates BETWEEN its knots.  The solver holds the rows of its NLP at their own times only (dynamics
 * every dt_dyn, range of motion every dt_rom, terrain at the foot nodes, forces at the force nodes); the rows the robot executes
 * lie in between.  For B windows at once (k_plan_check, one workgroup per window; the rule: plan_check.py) check row k of a plan,
 * at the plan time min(k / hz, T) of CSV row k, has 27 columns:
 *   0         the time stamp of CSV row k (t0 + k / hz, qtos_sample_csv's to the bit)
 *   1 ..  3   the angular dynamics rows  I_w wd + w x (I_w w) - sum f_e x (r - p_e)   [N m], signed
 *   4 ..  6   the linear dynamics rows   m a + m g e_z - sum f_e                       [N], signed
 *   7 .. 18   range of motion, feet FL FR HL HR x 3 axes: max(lo - g, g - hi) of g = R^T (p_e - r) against nominal_stance -+
 *             max_dev; negative: inside                                                [m]
 *  19 .. 22   clearance of the feet z - h(x, y) under the handle's terrain_mode and the window's map (no maps: flat ground) [m]
 *  23 .. 26   force excess of the feet; in a stance polynomial of the foot's motion the largest excess of the NLP's five force
 *             rows (normal force in [0, f_max], the four rows of the friction pyramid) with the terrain basis at the foot's
 *             position, in a swing polynomial max |f_i|                                [N]
 * A row exactly on a phase switch belongs to the earlier polynomial (qtos_sample_csv's rule).  The summary has five records per
 * window, the families dyn_ang (max |columns 1 .. 3|), dyn_lin (max |4 .. 6|), rom (max(7 .. 18, 0)), terrain (|clearance| of a
 * foot in stance, max(-clearance, 0) of one in swing) and force (max(23 .. 26, 0)): the largest violation over the window's
 * rows, the lowest row that attains it and the number of rows with a violation > tol[family].  A non-finite column counts as
 * +inf.  A window without rows has max -inf, row -1, count 0.  The summary is a function of the table alone (no atomics). */
#define QTOS_CHECK_ACCUMULATE 1      /* flags: merge with the records in d_summary: max = max(old, new), row replaced only on a
                                        strictly greater max, count += new; a window without rows leaves its records alone */
#define QTOS_CHECK_COLS 27
#define QTOS_CHECK_FAMILIES 5
typedef struct QtosCheckRecord {
  double max;
  long long row, count;
} QtosCheckRecord;
typedef struct QtosPlanCheck {
  double hz;                    /* rows per second (<= 0: 1000) */
  int first_row;                /* first row where d_first_row is NULL; 0 .. 1000000 */
  int n_rows;                   /* rows per window in `rows` (>= 1), and the count where d_n_rows is NULL */
  double tol[5];                /* per family: a row counts where its violation is > tol */
  int flags;                    /* QTOS_CHECK_* */
} QtosPlanCheck;
/* nodes B x n_vars, t0 B; map_id B (NULL: map 0, or flat ground where the handle has no maps), first_row B and n_rows B
 * (NULL: the struct's; n clamped to 0 .. n_rows, a negative first_row taken as 0, as qtos_joint_rows does) and cursor B
 * (NULL: the summary's rows count from first_row; given: from cursor[b], the window's clock as qtos_stitch counts it: row =
 * cursor[b] + j) may be NULL.  rows B x n_rows x 27 and summary B x 5 records: either may be NULL, not both; rows behind a
 * window's count are not touched.
 * Device form: all pointers but `c` in device memory, one kernel queued on `stream`; no handle state is read or written but
 * the sampling tables, the model's constants and the terrain -- it may be queued while a call is open.  Host form: host
 * pointers, synchronous, through device buffers of its own (no -5); rows and summary are copied in and out whole.
 * Both: -1 on a null planner or required pointer, B < 1, n_rows < 1, first_row outside 0 .. 1000000, rows and summary both
 * NULL; -2 on a HIP error; -3 out of memory. */
int qtos_plan_check_device(QtosPlanner *p, int B, const QtosPlanCheck *c, const double *d_nodes, const double *d_t0,
                           const int *d_map_id /* may be NULL */, const int *d_first_row /* may be NULL */,
                           const int *d_n_rows /* may be NULL */, const long long *d_cursor /* may be NULL */,
                           double *d_rows /* may be NULL */, QtosCheckRecord *d_summary /* may be NULL */, void *stream);
int qtos_plan_check(QtosPlanner *p, int B, const QtosPlanCheck *c, const double *nodes, const double *t0, const int *map_id,
                    const int *first_row, const int *n_rows, const long long *cursor, double *rows, QtosCheckRecord *summary);

/* Rollout: the windows' robots as simulated rigid bodies.  Replaces what scripts/run.py asks its simulator for once per tick (step
 * the robot, read traj_vec back) for B windows at once, for a user without PyBullet: the planner's own model -- ONE rigid body
 * with mass, inertia_b and gravity, the plan's forces at the plan's feet -- integrated forward under a plan, with a PD wrench
 * towards the plan and an optional push (k_rollout, one workgroup per window; the rule: rollout.py).  It has no contacts, no
 * legs' inertia and no friction limits on the applied forces.  Per row k of a window, at the plan time min(k / hz, T), with c
 * qtos_sample_csv's row: r_p = c[1:4], v_p = c[19:22], q_p the quaternion (x, y, z, w) of Rz Ry Rx of c[4:7], w_p = M(th) thd
 * the world angular velocity, F = ff_scale sum f_e, tau_p = ff_scale sum (p_e - r_p) x f_e about the PLANNED CoM.
 * State of a window, 13 doubles in d_state: r[3], v[3] (world), q[4] body to world (x, y, z, w), w_b[3] (body frame).  One tick
 * takes `substeps` steps of h = 1 / (hz substeps) with the row's quantities held; every step, from the state at its start:
 *   e = r - r_p;  F_fb = clip(-(kp_lin e) - kd_lin (v - v_p), +-f_fb_max) per component (a limit of 0: no clip)
 *   a = ((F + F_fb) + F_push) / m_s - g e_z, m_s = mass mass_scale[b];  R = R(q);  q_e = q_p (x) conj(q), negated if its w < 0
 *   tau_fb = clip(kp_ang 2 vec(q_e) + kd_ang (w_p - R w_b), +-t_fb_max);  tau = ((tau_p - e x F) + tau_fb) + tau_push
 *   v += h a, then r += h v;  w_b += h Ib_s^-1 (R^T tau - w_b x Ib_s w_b), Ib_s = mass_scale[b] inertia_b, Ib_s^-1 =
 *   inertia_b_inv / mass_scale[b];  q = (q + (h / 2) q (x) (w_b, 0)) / |.| with the new w_b
 * one rounded operation after the other in rollout.py's order: only +, -, x, / and sqrt.  The push, push[b] = (F_push, tau_push)
 * in the world, acts on the ticks c with push_from <= c < push_from + push_ticks, c = count[b] + j the window's running tick
 * count (count[b] += n behind the call).
 * Row k holds the state at the START of tick k; behind a call over n rows the carried state is the state at row first + n.  With
 * QTOS_ROLLOUT_INIT the state is first set from row `first` of the plan (r_p, v_p, q_p, R^T w_p); without it the carried state
 * is used: the body does not jump when the plan under it changes.  The flag holds for every window of the call that has rows;
 * a window whose carried word has QTOS_ROLLOUT_PENDING set is set on its plan likewise, by the first call that gives it rows,
 * which clears the bit (a window with n = 0 keeps it): for windows that get their first rows in different calls.
 * Outputs per row, in qtos_track's addressing (table, or ring with capacity / cursor):
 *   meas    the row qtos_track / qtos_start_feedback read: position, Euler angles (roll = atan2(R21, R22), pitch = asin(clip(-R20)),
 *           yaw = atan2(R10, R00) of R(q)), or with QTOS_ROLLOUT_QUAT position and q; the twelve joint angles are columns 1 .. 12
 *           of the same row of d_joint (qtos_joint_rows' rows, same addressing).  With d_joint NULL those columns are not touched
 *   rows    20 columns: 0 the time stamp (qtos_sample_csv's, to the bit), 1 .. 3 r, 4 .. 6 the Euler angles, 7 .. 9 v, 10 .. 12 R w_b,
 *           13 .. 16 q, 17 |e|, 18 2 |vec(q_e)| (about the angle between body and plan), 19 |F_fb| of the tick's first step
 *   status  bit 0 fallen: |e| > dev_max or column 18 > tilt_max (a limit of 0: never); bit 1 a non-finite state; both are kept in
 *           the window's carried word d_word[b]: the row that sets one and every later row carry it, take no step and repeat
 *           the frozen state (column 19 is 0, bits 3 and 4 are clear).  Bit 2 gimbal (the clip of the Euler extraction acts),
 *           bit 3 a feedback component was clipped in this tick, bit 4 the push acts in this tick */
#define QTOS_ROLLOUT_INIT 1        /* flags: the state is set from the plan's row `first` */
#define QTOS_ROLLOUT_QUAT 2        /* flags: meas rows carry the quaternion (19 doubles), as QTOS_TRACK_QUAT */
#define QTOS_ROLLOUT_PENDING 32    /* d_word[b], never a row's status: window b is set on its plan by its first call with rows */
#define QTOS_ROLLOUT_COLS 20
#define QTOS_ROLLOUT_STATE 13
typedef struct QtosRollout {
  double hz;                    /* rows per second (> 0) */
  int substeps;                 /* steps per tick, 1 .. 1000 */
  int first_row;                /* first row where d_first_row is NULL; 0 .. 1000000 */
  int n_rows;                   /* table mode: rows per window; both modes: the count where d_n_rows is NULL (>= 0) */
  long long capacity;           /* 0: table mode; > 0: rows per window in the rings */
  int flags;                    /* QTOS_ROLLOUT_* */
  double mass, gravity;         /* the body (mass > 0) */
  double inertia_b[9];          /* row-major, body frame */
  double inertia_b_inv[9];      /* its inverse, formed once on the host in float64 */
  double ff_scale;              /* the plan's forces are applied times this (1: as planned, 0: free fall) */
  double kp_lin[3], kd_lin[3];  /* N / m, N s / m, world axes */
  double kp_ang[3], kd_ang[3];  /* N m / rad, N m s / rad, world axes */
  double f_fb_max, t_fb_max;    /* clip of every feedback component (0: none) */
  double dev_max, tilt_max;     /* fallen beyond these (m, rad; 0: never) */
  long long push_from, push_ticks;   /* the ticks the push acts on (>= 0) */
} QtosRollout;
/* nodes B x n_vars, t0 B; first_row B and n_rows B may be NULL (n clamped to 0 .. n_rows or capacity, a window with n = 0 keeps its
 * state, count and word); cursor B, NULL in table mode; joint B x rows x 37, mass_scale B (NULL: 1) and push B x 6 may be NULL;
 * state B x 13, count B and word B in / out; meas B x rows x 18 (19 with QTOS_ROLLOUT_QUAT), rows B x rows x 20 (may be NULL),
 * status B x rows; rows = n_rows or capacity.
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream`, no handle state is read or written but the
 * sampling tables -- it may be queued while a call is open, in front of qtos_track_device with the same nodes, t0, n_rows and
 * cursor.  Host form: host pointers, synchronous, through device buffers of its own as qtos_track (no -5); the in / out arrays
 * and the outputs are copied in and out whole.
 * Both: -1 on a null planner, and with the reason in qtos_last_error on a null required pointer, B < 1, capacity < 0, a ring
 * without cursor, a table with n_rows < 1, n_rows < 0, first_row outside 0 .. 1000000, substeps outside 1 .. 1000, hz or mass not
 * > 0, a singular inertia_b, a negative push_from or push_ticks; -2 on a HIP error; -3 out of memory. */
int qtos_rollout_device(QtosPlanner *p, int B, const QtosRollout *s, const double *d_nodes, const double *d_t0,
                        const int *d_first_row /* may be NULL */, const int *d_n_rows /* may be NULL */,
                        const long long *d_cursor /* NULL in table mode */, const double *d_joint /* may be NULL */,
                        const double *d_mass_scale /* may be NULL = 1 */, const double *d_push /* may be NULL */,
                        double *d_state /* in/out */, long long *d_count /* in/out */, int *d_word /* in/out */, double *d_meas,
                        double *d_rows /* may be NULL */, int *d_status, void *stream);
int qtos_rollout(QtosPlanner *p, int B, const QtosRollout *s, const double *nodes, const double *t0, const int *first_row,
                 const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                 double *state, long long *count, int *word, double *meas, double *rows, int *status);

/* Rollout through the feet: qtos_rollout with its feedback wrench delivered by the feet that stand (k_rollout_feet, one workgroup
 * per window; the rule, with the order of every operation: rollout_feet.py).  qtos_rollout applies F_fb and tau_fb to the body as a
 * free wrench; a quadruped pushes only through its stance feet, and two point feet supply no moment about the line through them.
 * Per row, beside qtos_rollout's quantities: p_e and f_e the plan's foot positions and forces (CSV columns 7 .. 18 and 25 .. 36),
 * the stance flags as qtos_force_fit takes them, n their number, and the fit's load weights with g_e = f_e,z, the VERTICAL
 * component: w_e = max(n max(g_e, 0) / sum_S max(g, 0), w_min), all 1 where the sum is not > 0 (qtos_force_fit takes g_e along the
 * terrain normal; the rollout reads no terrain, and the two are equal on flat ground and on nearest-cell terrain).
 * Per step the lines of qtos_rollout hold but for a and tau:
 *   rho~ = (tau_fb / arm, F_fb), the clipped PD terms;  l_e = p_e - r with r the STATE's position;  d_e = l_e / arm
 *   M = sum_S w_e A~_e A~_e^T + damping n I6, A~_e = [skew(d_e); I3];  y = M^-1 rho~ by qtos_force_fit's unpivoted Cholesky (n = 0:
 *   y = 0);  df_e = w_e (y_ang x d_e + y_lin) for a stance foot, 0 for a swing foot;  f_a,e = ff_scale f_e + df_e
 *   QTOS_FEET_LIMIT: every STANCE foot's f_a is then limited by comparisons (a NaN stays a NaN): z = max(f_z, 0); f_max > 0: z =
 *   min(z, f_max); f_x and f_y clipped to +-mu z.  Against the vertical: the terrain normal only on flat and nearest-cell terrain
 *   F_a = ((f_a,0 + f_a,1) + f_a,2) + f_a,3;  tau_a = sum_e l_e x f_a,e in the same order
 *   a = (F_a + F_push) / m_s - g e_z;  tau = tau_a + tau_push (the levers are taken from the actual centre of mass)
 * With all gains 0, ff_scale 1 and no limit df = 0 exactly, and r, v are qtos_rollout's to the bit.
 * meas, rows, state, count and word are qtos_rollout's (column 19 of rows stays |F_fb|, the DESIRED force of the tick's first
 * step).  frows has 16 columns, with g_e = f_a,e - ff_scale f_e of the tick's first step:
 *   0 the time stamp;  1 .. 12 f_a [N];  13 |sum_S g_e - F_fb| [N];  14 |sum_S l_e x g_e - tau_fb| [N m];  15 sqrt(sum_S |g_e|^2) [N]
 * 13 and 14 are what the feet did not deliver.  A frozen row has 0 in 13 .. 15 and the plan's forces f_e in 1 .. 12.
 * status: qtos_rollout's bits, and bit 6 no stance foot in this row, bit 7 exactly two stance feet, bit 8 a comparison of the limit
 * acted in a step of this tick. */
#define QTOS_FEET_LIMIT 1            /* feet_flags: limit every stance force (no pulling, friction pyramid, force cap) */
#define QTOS_ROLLOUT_FEET_COLS 16
#define QTOS_ROLLOUT_NO_STANCE 64    /* status of a row; QTOS_ROLLOUT_PENDING (32) stays the carried word's alone */
#define QTOS_ROLLOUT_TWO_STANCE 128
#define QTOS_ROLLOUT_LIMITED 256
typedef struct QtosRolloutFeet {
  /* the body: QtosRollout's fields under their names, in its order and at its offsets -- the first sizeof(QtosRollout) bytes ARE a
   * QtosRollout, and a caller may fill them through a QtosRollout pointer */
  double hz;
  int substeps;
  int first_row;
  int n_rows;
  long long capacity;
  int flags;                    /* QTOS_ROLLOUT_* */
  double mass, gravity;
  double inertia_b[9];
  double inertia_b_inv[9];
  double ff_scale;
  double kp_lin[3], kd_lin[3];
  double kp_ang[3], kd_ang[3];
  double f_fb_max, t_fb_max;
  double dev_max, tilt_max;
  long long push_from, push_ticks;
  /* the feet */
  double arm;                   /* length the moment rows are divided by (> 0) [m] */
  double damping;               /* > 0 */
  double w_min;                 /* floor of the load weights, 0 < w_min <= 1 */
  double mu;                    /* friction coefficient of the limit (>= 0) */
  double f_max;                 /* cap of the vertical force of the limit [N] (<= 0: none) */
  int feet_flags;               /* QTOS_FEET_* */
} QtosRolloutFeet;
/* The arguments are qtos_rollout's, with frows B x rows x 16 (may be NULL) in front of status; both forms behave as
 * qtos_rollout's do (one kernel on `stream`; the host form synchronous through device buffers of its own).
 * Both: qtos_rollout's errors, and -1 with the reason in qtos_last_error on arm or damping not > 0, w_min outside (0, 1], mu < 0 or
 * not a number. */
int qtos_rollout_feet_device(QtosPlanner *p, int B, const QtosRolloutFeet *s, const double *d_nodes, const double *d_t0,
                             const int *d_first_row /* may be NULL */, const int *d_n_rows /* may be NULL */,
                             const long long *d_cursor /* NULL in table mode */, const double *d_joint /* may be NULL */,
                             const double *d_mass_scale /* may be NULL = 1 */, const double *d_push /* may be NULL */,
                             double *d_state /* in/out */, long long *d_count /* in/out */, int *d_word /* in/out */, double *d_meas,
                             double *d_rows /* may be NULL */, double *d_frows /* may be NULL */, int *d_status, void *stream);
int qtos_rollout_feet(QtosPlanner *p, int B, const QtosRolloutFeet *s, const double *nodes, const double *t0, const int *first_row,
                      const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                      double *state, long long *count, int *word, double *meas, double *rows, double *frows, int *status);

/* Force fit: the contact forces of every row made to supply the wrench the planned MOTION needs ("force distribution").  Between
 * its knots a plan's rows do not obey Newton's law (qtos_plan_check measures by how much); the motion is what the robot tracks, so
 * the forces give.  For B windows at once (k_force_fit, one workgroup per window; the rule, with the order of every operation of
 * the solve: force_fit.py), per row k at the plan time min(k / hz, T), with r, p_e, f_e and stance as the check row has them:
 *   rho_ang, rho_lin  the check row's columns 1 .. 3 and 4 .. 6 of the plan's own forces, formed with m_s = mass mass_scale[b] and
 *                     the inertia mass_scale[b] inertia_b, as qtos_rollout scales them
 *   S, n              the feet whose motion polynomial is a stance, and their number
 *   d_e = (p_e - r) / arm;  rho~ = (rho_ang / arm, rho_lin);  A~_e = [skew(d_e); I3]
 *   w_e = max(n max(g_e, 0) / sum_S max(g, 0), w_min), g_e = normal . f_e with the terrain basis at the foot (the first of the
 *         NLP's five force rows); all 1 where the sum is not > 0
 *   M = sum_S w_e A~_e A~_e^T + damping n I6;  y = M^-1 rho~ by an unpivoted Cholesky;  df_e = w_e A~_e^T y, e in S
 *   f_fit_e = f_e + df_e for e in S; a swing foot keeps the plan's force; n = 0: nothing is fitted
 * A fit row has 32 columns:
 *   0          the time stamp of CSV row k (t0 + k / hz, qtos_sample_csv's to the bit)
 *   1 .. 12    f_fit, feet FL FR HL HR x xyz, world frame                                                  [N]
 *  13 .. 15    the angular dynamics rows with f_fit in place of f, signed as check columns 1 .. 3 (rho - A df)  [N m]
 *  16 .. 18    the linear ones, as check columns 4 .. 6                                                    [N]
 *  19          sqrt(sum_S |df_e|^2)                                                                        [N]
 *  20 .. 31    tau_ff = -J^T R^T f_fit per leg, J the leg Jacobian of qtos_joint_rows at the joint angles in columns 1 .. 12 of the
 *              same row of d_joint (qtos_joint_rows' rows, same addressing); with d_joint NULL these columns are not touched  [N m]
 * and a status word: bit 0 no stance foot; bit 1 exactly two stance feet (two point feet cannot carry every moment: what remains
 * is the damped least-squares compromise); bit 2 a non-finite input or result -- then f_fit is the plan's force and columns
 * 13 .. 19 are NaN; bit 3 + e the fitted force of stance foot e exceeds the NLP's five force rows by more than excess_tol (the
 * check row's formula of column 23 + e on f_fit).  There are no inequality constraints inside the fit: the excess is measured
 * (qtos_force_qp below is the fit under those limits).
 * The summary has four QtosCheckRecords per window, the families res_ang (max |13 .. 15|), res_lin (max |16 .. 18|), change
 * (column 19) and excess (the largest positive excess over the stance feet), with qtos_plan_check's semantics: the largest
 * violation, the lowest row that attains it, the rows over tol[family]; non-finite counts as +inf; a window without rows has
 * -inf, -1, 0; no atomics.  Rows count from first (table) or from cursor[b], the window's clock (ring).
 * Addressing is qtos_joint_rows': capacity 0 a B x n_rows table, capacity > 0 a B x capacity ring at (cursor[b] + j) mod
 * capacity, cursor and t0 only read -- queued behind qtos_joint_rows_device and in front of qtos_stitch_device with the same
 * nodes, n_rows, t0 and cursor it fills a fit ring row for row with the CSV and joint rings. */
#define QTOS_FIT_ACCUMULATE 1        /* flags: merge with the records in d_summary, as QTOS_CHECK_ACCUMULATE */
#define QTOS_FIT_COLS 32
#define QTOS_FIT_FAMILIES 4
typedef struct QtosForceFit {
  double hz;                    /* rows per second (<= 0: 1000) */
  int first_row;                /* first row where d_first_row is NULL; 0 .. 1000000 */
  int n_rows;                   /* table mode: rows per window; both modes: the count where d_n_rows is NULL (>= 0) */
  long long capacity;           /* 0: table mode; > 0: rows per window in the rings */
  int flags;                    /* QTOS_FIT_* */
  double arm;                   /* length the moment rows are divided by (> 0) [m] */
  double damping;               /* > 0 */
  double w_min;                 /* floor of the load weights, 0 < w_min <= 1 */
  double excess_tol;            /* status bit 3 + e: excess > excess_tol [N] */
  double tol[4];                /* per family: a row counts where its violation is > tol */
  double hip[4][3];             /* the leg data as QtosJointRows has it; columns 20 .. 31 read lateral, l_upper and l_lower */
  double lateral[4];
  double l_upper, l_lower;      /* link lengths (> 0) */
  double knee_sign[4];
  double ee_shift;
} QtosForceFit;
/* nodes B x n_vars, t0 B; map_id B (NULL: map 0, or flat ground where the handle has no maps), first_row B, n_rows B, joint B x rows
 * x 37 and mass_scale B (NULL: 1) may be NULL; cursor B, NULL in table mode; rows B x rows x 32 with status B x rows, or summary
 * B x 4 records, may be NULL, not both (rows and status go together); rows = n_rows or capacity; rows behind a window's count are
 * not touched.
 * Device form: all pointers but `s` in device memory, one kernel queued on `stream`; no handle state is read or written but the
 * sampling tables, the model's constants and the terrain -- it may be queued while a call is open.  Host form: host pointers,
 * synchronous, through device buffers of its own (no -5); rows, status and summary are copied in and out whole.
 * Both: -1 on a null planner, and with the reason in qtos_last_error on a null required pointer, B < 1, rows without status or the
 * reverse, rows and summary both NULL, capacity < 0, a ring without cursor, a table with n_rows < 1, n_rows < 0, first_row outside
 * 0 .. 1000000, arm or damping not > 0, w_min outside (0, 1], excess_tol not a number, a link length <= 0; -2 on a HIP error; -3
 * out of memory. */
int qtos_force_fit_device(QtosPlanner *p, int B, const QtosForceFit *s, const double *d_nodes, const double *d_t0,
                          const int *d_map_id /* may be NULL */, const int *d_first_row /* may be NULL */,
                          const int *d_n_rows /* may be NULL */, const long long *d_cursor /* NULL in table mode */,
                          const double *d_joint /* may be NULL */, const double *d_mass_scale /* may be NULL = 1 */,
                          double *d_rows /* may be NULL */, int *d_status /* NULL iff d_rows is NULL */,
                          QtosCheckRecord *d_summary /* may be NULL */, void *stream);
int qtos_force_fit(QtosPlanner *p, int B, const QtosForceFit *s, const double *nodes, const double *t0, const int *map_id,
                   const int *first_row, const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale,
                   double *rows, int *status, QtosCheckRecord *summary);

/* Force QP: the force fit inside the friction pyramid -- the best wrench the stance feet can deliver without pulling, without
 * sliding and below the force cap.  For B windows at once (k_force_qp, one workgroup of 128 lanes per window, one lane per row;
 * the rule, with the order of every operation: force_qp.py).  Per row, with everything up to the fit's M, y and df_fit as
 * qtos_force_fit forms it, and the NLP's five force rows written as six rows per stance foot with the terrain basis at the foot,
 *   -n.f <= 0, n.f <= f_max, (t1 - mu n).f <= 0, -(t1 + mu n).f <= 0, (t2 - mu n).f <= 0, -(t2 + mu n).f <= 0    (G_e f_e <= h_e),
 * the problem in x = (df_e), e in S, c = damping n:
 *   minimise 1/2 |rho~ - sum_S A~_e df_e|^2 + 1/2 c sum_S |df_e|^2 / w_e   subject to   G_e (f_e + df_e) <= h_e, e in S
 * whose unconstrained minimiser is the fit.  Where the fit's forces obey every limit row the row is the fit's row (fit path).
 * Otherwise (limited path) the result is DEFINED as the central point of the barrier problem at the fixed weight mu_end, the
 * minimiser of the objective - mu_end sum log(h - G f): strictly feasible, a smooth function of the data, suboptimal by at most
 * 6 n mu_end; it is computed by a feasible-start primal-dual interior-point iteration (Mehrotra steps down to 10 mu_end, then
 * centering steps; one unpivoted 12 x 12 Cholesky per step) that stops at max |s z - mu_end| <= 1e-10 mu_end and |r_d|inf <=
 * 1e-9 (1 + |q|inf), or after max_iter steps -- then the row keeps its last iterate, which is feasible, and says so.
 * A row without a stance foot, a swing foot and a non-finite row behave as in qtos_force_fit.
 * Outputs per row: qtos_force_fit's 32 columns with f_qp in place of f_fit (13 .. 18 the dynamics rows with f_qp, 19 the size of
 * f_qp - f, 20 .. 31 tau_ff from f_qp), so a consumer of fit rows takes them as they are; 8 columns of the solve (qrows):
 *   0 steps taken (0 on the fit path)   1 max |s z - mu_end| / mu_end   2 |r_d|inf [N]   3 the smallest slack over the stance feet [N]
 *   4 the largest multiplier   5 sqrt(sum |f_qp - f_fit|^2) [N]   6 objective(f_qp) - objective(f_fit) >= 0 [N^2]
 *   7 the number of limit rows with slack <= act_tol
 * and a status word: bits 0 .. 2 as qtos_force_fit's; bit 3 + e foot e has a limit row with slack <= act_tol; bit 7 the cap of
 * max_iter steps was reached; bit 8 the row took the limited path.  The summary has four QtosCheckRecords per window: res_ang,
 * res_lin and change as qtos_force_fit's, and limited (column 5 of qrows), with qtos_plan_check's semantics and merge; no atomics.
 * Addressing, the device and host forms and the return codes are qtos_force_fit's; also -1 with the reason in qtos_last_error for
 * mu, f_max or mu_end not > 0, act_tol not a number, max_iter outside 1 .. 25. */
#define QTOS_QP_COLS 8
#define QTOS_QP_MAX_ITER 25
#define QTOS_QP_NO_STANCE 1          /* status bits of a force-QP row */
#define QTOS_QP_TWO_STANCE 2
#define QTOS_QP_NONFINITE 4
#define QTOS_QP_ACTIVE 8             /* << e: foot e has a limit row with slack <= act_tol */
#define QTOS_QP_CAP 128
#define QTOS_QP_LIMITED 256
typedef struct QtosForceQp {
  double hz;                    /* QtosForceFit's fields, in its order */
  int first_row;
  int n_rows;
  long long capacity;
  int flags;                    /* QTOS_FIT_* */
  double arm;
  double damping;
  double w_min;
  double excess_tol;            /* not read */
  double tol[4];                /* per family: res_ang, res_lin, change, limited */
  double hip[4][3];
  double lateral[4];
  double l_upper, l_lower;
  double knee_sign[4];
  double ee_shift;
  double mu;                    /* friction coefficient of the pyramid (> 0) */
  double f_max;                 /* cap of the normal force (> 0) [N] */
  double mu_end;                /* the barrier weight of the central point (> 0) [N^2] */
  double act_tol;               /* a limit row counts as active where its slack is <= act_tol [N] */
  int max_iter;                 /* 1 .. 25 */
} QtosForceQp;
int qtos_force_qp_device(QtosPlanner *p, int B, const QtosForceQp *s, const double *d_nodes, const double *d_t0,
                         const int *d_map_id /* may be NULL */, const int *d_first_row /* may be NULL */,
                         const int *d_n_rows /* may be NULL */, const long long *d_cursor /* NULL in table mode */,
                         const double *d_joint /* may be NULL */, const double *d_mass_scale /* may be NULL = 1 */,
                         double *d_rows /* may be NULL */, double *d_qrows /* may be NULL */, int *d_status /* NULL iff d_rows is NULL */,
                         QtosCheckRecord *d_summary /* may be NULL */, void *stream);
int qtos_force_qp(QtosPlanner *p, int B, const QtosForceQp *s, const double *nodes, const double *t0, const int *map_id,
                  const int *first_row, const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale,
                  double *rows, double *qrows, int *status, QtosCheckRecord *summary);

/* Rollout with the force QP: qtos_rollout_feet with qtos_force_qp's limited path in place of the comparisons of QTOS_FEET_LIMIT, in
 * every step of the simulated closed loop (k_rollout_qp, one workgroup per window; the rule, with the order of every operation:
 * rollout_qp.py).  Everything is qtos_rollout_feet's -- the inputs, the weights, the step's lines, the freeze, PENDING / INIT, the
 * columns of meas, rows and frows -- except the line that forms f_a.  Per step, with f0_e = ff_scale f_e, df_e, d_e, rho~ and n as
 * qtos_rollout_feet forms them and the six limit rows of qtos_force_qp in the basis of flat ground (the rollout reads no terrain):
 *   fit path      every stance foot's six values G (f0 + df) - h are <= 0:  f_a = f0 + df, qtos_rollout_feet's unlimited step to the
 *                 bit.  A NaN fails the comparison, takes the limited path and runs into the cap; the next row's freeze catches it
 *   limited path  f_a = f0 + x, x the central point at weight mu_end of qtos_force_qp's problem with d = d_e, w, rho~, c = damping n,
 *                 f = f0 and the fit df: strictly feasible, by that function's iteration and stopping rule
 * A per-step optimum is not a balance controller: the call reports what the limits cost the feedback, it cures nothing.
 * qrows has qtos_force_qp's 8 columns for the tick's FIRST step (on the fit path 0 but for columns 3 and 7, which come from the
 * fit's slacks; 0 on a row without a stance foot and on a frozen row).  status: qtos_rollout_feet's bits, with bit 8 (LIMITED) a step
 * of this tick took the limited path, and bit 9 (CAP) a step reached max_iter. */
#define QTOS_ROLLOUT_QP_COLS 8
#define QTOS_ROLLOUT_CAP 512
typedef struct QtosRolloutQp {
  /* QtosRolloutFeet's fields under their names, in its order and at its offsets */
  double hz;
  int substeps;
  int first_row;
  int n_rows;
  long long capacity;
  int flags;                    /* QTOS_ROLLOUT_* */
  double mass, gravity;
  double inertia_b[9];
  double inertia_b_inv[9];
  double ff_scale;
  double kp_lin[3], kd_lin[3];
  double kp_ang[3], kd_ang[3];
  double f_fb_max, t_fb_max;
  double dev_max, tilt_max;
  long long push_from, push_ticks;
  double arm;
  double damping;
  double w_min;
  double mu;                    /* friction coefficient of the pyramid (> 0) */
  double f_max;                 /* cap of the normal force (> 0) [N] */
  int feet_flags;               /* not read */
  /* the QP */
  double mu_end;                /* the barrier weight of the central point (> 0) [N^2] */
  double act_tol;               /* a limit row counts as active where its slack is <= act_tol [N] */
  int max_iter;                 /* 1 .. 25 */
} QtosRolloutQp;
/* The arguments are qtos_rollout_feet's, with qrows B x rows x 8 (may be NULL) behind frows; both forms behave as qtos_rollout_feet's
 * do.  Both: qtos_rollout_feet's errors, and -1 with the reason in qtos_last_error on mu, f_max or mu_end not > 0, max_iter outside
 * 1 .. 25, act_tol not a number. */
int qtos_rollout_qp_device(QtosPlanner *p, int B, const QtosRolloutQp *s, const double *d_nodes, const double *d_t0,
                           const int *d_first_row /* may be NULL */, const int *d_n_rows /* may be NULL */,
                           const long long *d_cursor /* NULL in table mode */, const double *d_joint /* may be NULL */,
                           const double *d_mass_scale /* may be NULL = 1 */, const double *d_push /* may be NULL */,
                           double *d_state /* in/out */, long long *d_count /* in/out */, int *d_word /* in/out */, double *d_meas,
                           double *d_rows /* may be NULL */, double *d_frows /* may be NULL */, double *d_qrows /* may be NULL */,
                           int *d_status, void *stream);
int qtos_rollout_qp(QtosPlanner *p, int B, const QtosRolloutQp *s, const double *nodes, const double *t0, const int *first_row,
                    const int *n_rows, const long long *cursor, const double *joint, const double *mass_scale, const double *push,
                    double *state, long long *count, int *word, double *meas, double *rows, double *frows, double *qrows, int *status);

/* Goals of receding windows from their global paths: where the next plan goes.  Replaces Global_Planner.update / spine_step
 * (QTOS/planner.py:139-161, 195-230) and Combiner.plan_init / spine_step (QTOS/combiner.py:137-212, 223-225) for B windows at
 * once: a window's A* "spine" -- two cubic splines X_p, Y_p over one set of knots -- is read one horizon ahead of the new plan's
 * start, the displacement from a base point is clipped to step_size per axis, and the goal height is the terrain under the goal
 * + z_offset.  One lane per window (k_path_goal); per window b, with p its path and H(x, y) the height rule below:
 *   lt = clock[b] + offset[b]                          the plan time of the new plan's row 0;  tf = lt + horizon
 *   sx = X_p(tf), 0.0 unless |sx| > tol;  sy likewise;  gz = H(sx, sy) + z_offset
 *   clamp_x: sx = robot_goal[p][0] where sx is larger      (Combiner.spine_step; behind gz, as the reference does)
 *   base 0 (spine, Global_Planner.update): (X_p(lt), Y_p(lt), H(X_p(lt), Y_p(lt)) + z_offset), without the tol rule
 *   base 1 (state, plan_init and spine_step(com, t)): start[b][0:3]
 *   goal_out[b] = base + clip((sx, sy, gz) - base, -step_size, +step_size)       per component; a NaN stays a NaN
 *   bit 0: t_end[p] < lt - t_stop   (t_end the path's last knot; the reference stops with t_stop = 5 + lookahead / hz)
 *   bit 1: stop_dist > 0 and sqrt(dx dx + dy dy) < stop_dist, (dx, dy) = start[b][0:2] - goal_out[b][0:2]  (scripts/main.py:40-46)
 *   done[b] |= bits (sticky);  hold_done: goal_out[b] = start[b][0:3] where done[b] is now non-zero -- the window stands still
 *   instead of following the spline's extrapolation beyond the path's end;  advance_clock: clock[b] = lt.
 * A spline is evaluated as scipy's CubicSpline evaluates it, to the bit: piece i = the number of knots <= t, less one, kept
 * within 0 .. n - 1 (times before the first knot use piece 0, times at or beyond the last knot piece n - 1), s = t - x[i],
 * res = 0, z = 1, four times res = res + c[3 - kp][i] * z, z = z * s -- every operation one rounded IEEE double operation.
 * H: row = floor((y + origin_y) / cell), col = floor((x + origin_x) / cell); a negative index down to -rows / -cols wraps as
 * Python's does; anything else (out of range, non-finite) reads the cell [rows - 1][cols / 2].  The numpy statement of all of
 * this is global_planner.path_goal, which the kernel equals to the bit. */
typedef struct QtosPathGoal {
  double horizon;              /* seconds the spine is read ahead of the plan's start (the reference: 5.0)      */
  double step_size;            /* clip of the goal's displacement per axis (>= 0)                               */
  double tol;                  /* a spine coordinate within tol of zero is zero (the reference: 1e-5)           */
  double z_offset;             /* height of the base above the terrain (the reference: 0.24)                    */
  double cell, origin_x, origin_y;  /* of the height grids (> 0; the reference: 0.1, 1.0, 1.0)                  */
  double t_stop, stop_dist;    /* the done bits (stop_dist <= 0: no bit 1)                                      */
  int base;                    /* 0 spine, 1 state                                                              */
  int clamp_x, advance_clock, hold_done;
  int n_paths, max_pieces;     /* of the path table (>= 1)                                                      */
  int n_maps, rows, cols;      /* of the height grids (>= 1 where a grid is given)                              */
} QtosPathGoal;
/* The path table (global_planner.path_table): knots n_paths x (max_pieces + 1), the rows of shorter paths padded with their
 * last knot; coef n_paths x 2 x 4 x max_pieces, X then Y, scipy's layout (coef[p][a][k][i] multiplies (t - x[i])^(3 - k)),
 * padding zero; n_pieces n_paths (values outside 1 .. max_pieces are read as the nearest of the two); robot_goal n_paths x 3
 * (may be NULL without clamp_x).  path_id B (may be NULL: window b follows path b, which needs n_paths >= B; ids outside the
 * table are read as the nearest path); height_yx n_maps x rows x cols (may be NULL: every height is 0) with map_id B (may be
 * NULL: map 0; ids outside are read as the nearest map); clock B (in / out: written only with advance_clock); offset B (may be
 * NULL: 0; in a loop, offset_out of qtos_handover*); start B x 24 (in a loop, start_out of qtos_handover*; may be NULL where
 * nothing reads it: base 0, stop_dist <= 0 and hold_done off); goal_out B x 3; done B (in / out, may be NULL: no done bits are
 * kept -- hold_done needs it).
 * Device form: all pointers but `g` in device memory, one kernel queued on `stream`; directly behind qtos_handover_device on the
 * same stream d_start / d_offset may be its d_start_out / d_offset_out.  No handle state is read or written -- launch pattern,
 * totals and report flag stay, a plan call behind it returns the bits it would have returned without it, and it may be queued
 * while a call is open.  Host form: host pointers, synchronous, through device buffers of its own as qtos_stitch (no -5); the
 * result is what the device form leaves.
 * Both: -1 on bad arguments, with no kernel launched -- a null planner or required pointer, B < 1, n_paths or max_pieces < 1,
 * path_id NULL with n_paths < B, a height grid with n_maps, rows or cols < 1, cell <= 0, step_size < 0 (or any of the two not a
 * number), base outside 0 / 1, clamp_x without robot_goal, hold_done without done, start NULL where it is read; -2 on a HIP
 * error; -3 out of memory. */
int qtos_path_goal_device(QtosPlanner *p, int B, const QtosPathGoal *g, const double *d_knots, const double *d_coef,
                          const int *d_n_pieces, const double *d_robot_goal /* may be NULL */, const int *d_path_id /* may be NULL */,
                          const double *d_height_yx /* may be NULL */, const int *d_map_id /* may be NULL */, double *d_clock /* in/out */,
                          const double *d_offset /* may be NULL */, const double *d_start /* may be NULL */, double *d_goal_out,
                          int *d_done /* in/out, may be NULL */, void *stream);
int qtos_path_goal(QtosPlanner *p, int B, const QtosPathGoal *g, const double *knots, const double *coef, const int *n_pieces,
                   const double *robot_goal, const int *path_id, const double *height_yx, const int *map_id, double *clock,
                   const double *offset, const double *start, double *goal_out, int *done);

/* The global paths of receding windows, planned on the device: what qtos_path_goal* reads.  Replaces PATH_Solver (QTOS/planner.py:
 * 282-457; PATH_Solver.solve :422-457 when maps or goals change) for B windows at once, one wavefront per window (k_path_plan):
 * A* over the window's boolean map from its start point to its robot goal, then every second cell of the path a point of two
 * not-a-knot cubics X(t), Y(t) over T = |start - goal| / step_size * 10 seconds.  The numpy statement of all of it is
 * global_planner.path_plan (path_cells, spine_fit), which the kernel equals to the bit:
 *   cells: (floor((y + origin_y) / cell), floor((x + origin_x) / cell)); 4 neighbours in the order (0,1), (0,-1), (1,0), (-1,0);
 *   blocked where bool_map > height_bound; g + 1 per step, f = g + sqrt(drow^2 + dcol^2); the open list is popped in the order
 *   of (f, (row, col)); a cell is pushed again where g < gscore or it has no entry in the open list (PATH_Solver.astar,
 *   statement by statement; a start cell outside the grid is expanded once and never indexed)
 *   points: sub = path[::2]; x = col * cell - origin_x over sub, then the last cell's col * cell without the shift (sic); y from
 *   the rows; n = len(sub) pieces over the knots i * (T / n), the last one T
 *   splines: scipy's not-a-knot system by a fixed elimination (n = 1 the line, n = 2 the parabola, n >= 3 the Thomas recurrence)
 * status[b]: 0 found; 1 no path (the open list ran empty, or a start / goal cell that is not finite or no int32); 2 the path has
 * more than max_cells cells (n_cells[b] is its length); 3 the open list would exceed max_open entries, or more than
 * 4 * rows * cols + 4 pops happened; 4 T is not > 0.  A window whose status is not 0 gets the one-piece constant spine at its
 * start point over the knots (0, 0), and with set_done bit 2 (value 4) of done[b]: k_path_goal with hold_done then keeps it on
 * its start. */
typedef struct QtosPathPlan {
  int rows, cols;              /* of the boolean maps (rows * cols <= 16384)                                     */
  double cell, origin_x, origin_y;  /* of the maps (cell > 0; the reference: 0.1, 1.0, 1.0)                      */
  double height_bound;         /* a cell is blocked where its value is larger (the reference: 0.2)               */
  double step_size;            /* of T (> 0)                                                                     */
  int max_cells;               /* longest path kept (1 .. min(2 * max_pieces, 16384))                            */
  int max_open;                /* longest open list (1 .. 4096)                                                  */
  int max_pieces;              /* of the path table written (>= 1)                                               */
  int n_maps;                  /* >= 1                                                                           */
  int set_done;                /* set bit 2 of done where status != 0 (needs done)                               */
} QtosPathPlan;
/* bool_maps n_maps x rows x cols doubles; map_id B (may be NULL: map 0; ids outside are read as the nearest map); start
 * B x QTOS_START_DOUBLES (only [0], [1] are read: the window's x, y); robot_goal B x 3 (only [0], [1] are read; the same array
 * is the table's robot_goal, window b following path b).  Written: knots B x (max_pieces + 1), coef B x 2 x 4 x max_pieces and
 * n_pieces B -- the path table of qtos_path_goal*, n_paths = B, padded as there; cells B x max_cells x 2 (row, col; padding 0;
 * may be NULL); n_cells B; status B; done B (in / out; may be NULL without set_done).
 * Device form: all pointers but `g` in device memory, one kernel queued on `stream`; no handle state is read or written, and it
 * may be queued while a call is open.  Host form: host pointers, synchronous, through device buffers of its own (no -5).
 * Both: -1 on a null planner; -2 on any other bad argument, with no kernel launched and the reason in qtos_last_error -- a null
 * `g` or required pointer, B < 1, rows or cols < 1, rows * cols > 16384, max_open outside 1 .. 4096, max_pieces < 1, max_cells
 * outside 1 .. min(2 * max_pieces, 16384), n_maps < 1, cell or step_size not > 0, a height_bound that is not a number, set_done
 * without done -- and on a HIP error; -3 out of memory. */
int qtos_path_plan_device(QtosPlanner *p, int B, const QtosPathPlan *g, const double *d_bool_maps, const int *d_map_id /* may be NULL */,
                          const double *d_start, const double *d_robot_goal, double *d_knots, double *d_coef, int *d_n_pieces,
                          int *d_cells /* may be NULL */, int *d_n_cells, int *d_status, int *d_done /* in/out, may be NULL */, void *stream);
int qtos_path_plan(QtosPlanner *p, int B, const QtosPathPlan *g, const double *bool_maps, const int *map_id, const double *start,
                   const double *robot_goal, double *knots, double *coef, int *n_pieces, int *cells, int *n_cells, int *status, int *done);

/* The boolean maps of receding windows from their heightfields, on the device: what qtos_path_plan* reads as bool_maps.  Replaces
 * PATH_MAP (QTOS/generateHeightField.py:172-404: probe_map queues a (start, goal) patch two cells apart wherever an obstacle is
 * near, 32 `docker exec ./main` workers solve the patches, worker_f stamps the exit codes into the map) for n_maps maps at once,
 * in two steps with the batched solve that already exists between them, all on one stream:
 *   map_yx --qtos_probe_device--> start N x 24, goal N x 3, map_id N --qtos_plan_batch_device--> status N
 *          --qtos_probe_stamp_device--> bool_maps --qtos_path_plan_device--> ...
 * The host reads ONE word in between: N = offsets[n_maps], the number of problems, to size the plan call or calls (a handle
 * solves up to max_batch problems per call).  The numpy statement of both steps is feasibility.probe_table / round2 /
 * stamp_table, which the kernels equal to the bit.
 * Probe (k_probe_count, k_probe_scan, k_probe; one wavefront per map).  Per map the patches of probe_map in queue order: row
 * r = 0 .. rows - 1 outside, j = 0 .. cols / 2 - 2 inside, start cell (r, 2 j), goal cell (r, 2 j + 2); a patch is queued where
 * neighbors_danger_test answers true for its start or its goal cell: the eight neighbours in the order (1,0), (-1,0), (0,1),
 * (0,-1), (1,1), (1,-1), (-1,-1), (-1,1) (row, column), false at the first one outside the map, true at the first one inside it
 * that is > 0 (a NaN is not).  The lists of the maps are concatenated, map 0's first; no atomics decide where a patch goes.
 * Coordinates, every operation one rounded IEEE double operation, with res = cell * (1 / scale), s = (multi_map_shift - 1) *
 * origin_shift and round2 = Python's round(v, 2):
 *   x_start = ((-res * (cols / 2)) - res / 2) + s     for x AND y (sic: both from the number of columns)
 *   x_goal  = ((-res * (cols / 2)) + res / 2) + s
 *   y_r: y <- round2(y + res) from x_start, once per row;  X_0 = round2(x_start + res), X_1 = round2(x_goal + 2 res),
 *   X_(j+1) = round2(X_j + 2 res): patch (r, j) starts at (X_j, y_r) and goes to (X_(j+1), y_r)
 *   round2(v): p = v * 100, e = fma(v, 100, -p) its exact error, k = rint(p); where |p - k| = 0.5 and e != 0,
 *   k = floor(p) + (e > 0); k / 100
 * start[i] = (X_j, y_r, z + z_offset), Euler angles 0, the feet nominal_stance[e] + (X_j, y_r, z) in the order FL FR HL HR,
 * velocities 0; goal[i] = (X_(j+1), y_r, z_goal + z_offset); z, z_goal the heights of the start and the goal cell; map_id[i] = the
 * map: map m of the call is heightfield m of the handle (qtos_set_heightfields with the same maps in the solver's orientation).
 * An all-zero map has no patch (the reference's check_flat_ground short-cut).
 * Stamp (k_probe_stamp; one wavefront per map, one lane per cell in turn).  A cell holds what the LAST patch in queue order
 * that writes it leaves: a patch with status 0 writes 0 to its start cell, the cell right of it and its goal cell; any other
 * status writes 1 to the diamonds |a| + |b| <= 3 scale round the start cell and round the goal cell, clipped to the map; a cell
 * nothing writes is 0. */
typedef struct QtosProbe {
  int rows, cols;              /* of the maps (cols >= 2, rows * cols <= 16384: the limit of qtos_path_plan*)    */
  int n_maps;                  /* 1 .. 16777216; n_maps * rows * (cols / 2 - 1) fits an int                      */
  double cell;                 /* of the maps at scale 1 (> 0; the reference: 0.1)                               */
  int scale;                   /* 1 .. 4: the cell is cell * (1 / scale), the diamond's radius 3 * scale         */
  int multi_map_shift;         /* >= 1 (the reference: the number of tiles of the map)                           */
  double origin_shift;         /* the reference: 1.0                                                             */
  double z_offset;             /* height of the base above the terrain (the reference: 0.24)                     */
  double nominal_stance[QTOS_NEE][3];  /* FL FR HL HR (the reference: (+-0.21, +-0.19, 0.0))                     */
} QtosProbe;
/* map_yx n_maps x rows x cols doubles (heights, row = y index, as the maps of qtos_path_goal*); capacity: the number of problems
 * the arrays patch, start, goal and map_id have room for (>= 0).  Written: offsets n_maps + 1 ints (exclusive prefix sums of the
 * maps' patch counts: offsets[0] = 0, offsets[n_maps] = N) and slot n_maps x rows x (cols / 2 - 1) ints (a patch's index i, or
 * -1), both whole; patch N x 3 ints (map, row, start column), start N x QTOS_START_DOUBLES, goal N x 3 and map_id N for the
 * patches with i < capacity, and nothing beyond them.  offsets, slot and patch are required (patch with capacity 0 is not
 * written, but not NULL); start, goal and map_id may each be NULL: that array is not written.  Where offsets[n_maps] > capacity
 * the caller allocates arrays of offsets[n_maps] problems and calls again: the first capacity problems are already right, and the
 * second call writes the same bits.
 * qtos_probe_stamp*: offsets, slot as a probe call left them; patch may be NULL: it is not read (the kernel finds the patches
 * through slot; the argument keeps the probe's arrays together in a call); status offsets[n_maps] ints (status_out of qtos_plan_batch*: 0 solved);
 * bool_maps n_maps x rows x cols doubles of 0.0 / 1.0, written whole: bool_maps of qtos_path_plan*.  Only rows, cols, n_maps
 * and scale of `g` are read by the stamp, and all of `g` is checked.
 * Device forms: all pointers but `g` in device memory, kernels queued on `stream`; no handle state is read or written, and they
 * may be queued while a call is open.  Host forms: host pointers, synchronous, through device buffers of their own as
 * qtos_path_plan (no -5); the result is what the device forms leave; qtos_probe_stamp reads offsets[n_maps] to size status.
 * All: -1 on a null planner; -2 on any other bad argument, with no kernel launched and the reason in qtos_last_error -- a null
 * `g` or required pointer, cols < 2, rows < 1, rows * cols > 16384, n_maps outside 1 .. 16777216 or too many for an int of
 * slots, scale outside 1 .. 4, multi_map_shift < 1, cell not > 0, an origin_shift, z_offset or stance that is not a number,
 * capacity < 0 -- and on a HIP error; -3 out of memory. */
int qtos_probe_device(QtosPlanner *p, const QtosProbe *g, const double *d_map_yx, int capacity, int *d_offsets, int *d_slot, int *d_patch,
                      double *d_start /* may be NULL */, double *d_goal /* may be NULL */, int *d_map_id /* may be NULL */, void *stream);
int qtos_probe(QtosPlanner *p, const QtosProbe *g, const double *map_yx, int capacity, int *offsets, int *slot, int *patch, double *start,
               double *goal, int *map_id);
int qtos_probe_stamp_device(QtosPlanner *p, const QtosProbe *g, const int *d_offsets, const int *d_slot, const int *d_patch /* may be NULL */,
                            const int *d_status, double *d_bool_maps, void *stream);
int qtos_probe_stamp(QtosPlanner *p, const QtosProbe *g, const int *offsets, const int *slot, const int *patch, const int *status,
                     double *bool_maps);

/* The randomised terrain of n_maps windows, on the device: what qtos_set_heightfields_device, qtos_probe* and qtos_path_goal*
 * read, made from base grids and one seed per map.  Replaces Height_Map_Generator.__init__ with randomize_env = True
 * (QTOS/generateHeightField.py:563-567: random_map_shift :648-690, random_height_shift :692-730) and, with n_shift = 1 and
 * n_height = 0 on the current maps and `draws` carried over, Height_Map_Generator.update() (:584-588).  The reference draws from
 * python's module-level `random`; map m here owns the stream of random.seed(seed[m]), and the kernel (k_terrain_env, one
 * workgroup per map) equals the numpy statement of the rule, heightfield.random_env_table, to the bit -- and with it the map the
 * reference leaves behind random.seed(seed[m]).  Per map, with base = base_yx[base_id[m]] (rows x cols, row = y index):
 *   stream   MT19937 seeded by init_by_array on the 32-bit words of seed[m], low word first (one word below 2^32, else two), its
 *            first draws[m] outputs discarded.  random() = ((u >> 5) * 2^26 + (u' >> 6)) / 2^53 from two outputs;
 *            uniform(a, b) = a + (b - a) * random(), product and sum rounded one by one (no fma); choice among n items: the
 *            top bit_length(n) bits of an output, redrawn while >= n.
 *   shifts   n_shift choices of a direction for the solver's copy -- consumed, the reference rebuilds that copy from the map --,
 *            then n_shift for the map, from (left, right, up, down), or from (up, down) where climb != 0; left / right roll
 *            the columns by -1 / +1, up / down the rows by -1 / +1, with wrap-around: one net roll.
 *   heights  n_height passes over the solver's copy (its list of levels alone: only the number of draws matters), then n_height
 *            over the map.  A pass takes the ascending distinct values != 0 (-0.0 is ground) and per such level h, in order,
 *            draws d = uniform(-delta, delta) and c = choice(0, 1, 2); the cells that equal h as the map stands at that moment
 *            get + d (c = 0), - d (c = 1) or nothing.  Levels that meet move as one from then on; one that lands on 0 stays.
 * Written per map: map_yx[m] rows x cols; height_xy[m] cols x rows (may be NULL), the solver's orientation: height_xy[m][x][y] =
 * map_yx[m][y][x - 1], row x = 0 zero (heightfield.towr_map); draws[m] (in/out, may be NULL: nothing is discarded, nothing
 * written) moved on by the outputs consumed; status[m]: 0 ok, 1 more than QTOS_ENV_MAX_LEVELS distinct levels, 2 draws[m]
 * negative or above QTOS_ENV_MAX_DRAWS on entry, 3 a NaN in the base grid, 4 base_id[m] outside 0 .. n_base - 1 (looked for in
 * the order 2, 4, 3, 1).  A map with a non-zero status keeps map_yx[m], height_xy[m] and draws[m] as they were. */
#define QTOS_ENV_MAX_LEVELS 64
#define QTOS_ENV_MAX_DRAWS (1 << 24)
#define QTOS_ENV_LDS_BYTES 3568      /* k_terrain_env's LDS: the generator's 624 words, two level lists, a reduction's partials */
typedef struct QtosTerrainEnv {
  int n_maps;                  /* 1 .. 16777216                                                                  */
  int n_base;                  /* base grids (>= 1; without base_id: >= n_maps)                                  */
  int rows, cols;              /* of every grid (>= 1, rows * cols <= 16777216)                                  */
  int n_shift;                 /* 0 .. 1048576 (the reference: 10 * mesh_scale; update(): 1)                     */
  int n_height;                /* 0 .. 1024 (the reference: 10; update(): 0)                                     */
  int climb;                   /* != 0: directions up / down only (climb_map_check: a climb_1 or climb_2 tile)   */
  double delta;                /* finite, >= 0 (the reference: 0.005)                                            */
} QtosTerrainEnv;
/* Device form: base_yx n_base x rows x cols doubles, base_id n_maps ints (may be NULL: map m reads base m; an entry outside
 * 0 .. n_base - 1 ends its map with status 4), seed n_maps 64-bit words, draws n_maps ints, map_yx, height_xy, status as above, all in device
 * memory; one kernel queued on `stream`; no handle state is read or written, and it may be queued while a call is open.  Host
 * form: host pointers, synchronous, through device buffers of its own (no -5); what the kernel does not write comes back as it
 * was; a base_id entry outside 0 .. n_base - 1 is an argument error there.
 * Both: -1 on a null planner; -2 on any other bad argument, with no kernel launched and the reason in qtos_last_error -- a null
 * `g` or required pointer, n_maps, n_base, rows or cols < 1 or beyond the limits above, n_base < n_maps without base_id,
 * n_shift or n_height negative or beyond the limits, a delta that is negative, infinite or not a number, an output (draws,
 * map_yx, height_xy, status) that overlaps any other array of the call -- and on a HIP error; -3 out of memory. */
int qtos_terrain_env_device(QtosPlanner *p, const QtosTerrainEnv *g, const double *d_base_yx, const int *d_base_id /* may be NULL */,
                            const unsigned long long *d_seed, int *d_draws /* in/out, may be NULL */, double *d_map_yx,
                            double *d_height_xy /* may be NULL */, int *d_status, void *stream);
int qtos_terrain_env(QtosPlanner *p, const QtosTerrainEnv *g, const double *base_yx, const int *base_id, const unsigned long long *seed,
                     int *draws, double *map_yx, double *height_xy, int *status);

/* The plan as the text file the reference copies out of its container (`docker cp <id>:.../build/traj.csv ./data/traj/towr.csv`,
 * scripts/main.py:90-92; consumers scripts/run.py:129-137, QTOS/combiner.py:263-274): rows is n_rows x 37 (one plan of
 * qtos_sample_csv), every number printed as the solver's C++ stream prints it (default precision 6 = printf "%g"), comma
 * separated, no header.  Host only, needs no planner and no GPU.  n_threads <= 0: chosen from n_rows (at most 8).
 * Returns 0, -1 bad arguments, -2 the file cannot be opened, -3 a short write. */
int qtos_write_csv(const char *path, const double *rows, int n_rows, int n_threads);

int qtos_plan_submit(QtosPlanner *p, int B, const double *d_start, const double *d_goal,
                     const int *d_map_id, const double *d_warm, double *d_nodes_out,
                     int *d_status_out, int *d_iters_out, double *d_viol_out, void *stream);
int qtos_plan_poll(QtosPlanner *p, int *done);
int qtos_plan_wait(QtosPlanner *p);
/* Rounds 3 - 5: upper limit of the iterations qtos_plan_submit queues "blind" -- BOTH solve kernels per iteration, as many
 * iterations as the previous call needed (measured slower than the informed loop: a blind iteration pays for launches
 * without work).  Default 1 = off; a limit above 1 replaces the launch pattern for this handle. */
int qtos_set_speculation(QtosPlanner *p, int max_blind_iterations);
/* The launch pattern of qtos_plan_submit (above) on / off for this handle (default on; off also forgets what was learnt:
 * the next call queues its first iteration and the host reads the counts in front of every further launch, as in rounds 1 - 5). */
int qtos_set_pattern_speculation(QtosPlanner *p, int on);
/* The environment switches this handle runs with, as text ("QTOS_KKT=0 QTOS_LANES=1 ..."): at most n - 1 characters and a
 * terminating zero into buf; returns the length of the full text.  Read once by qtos_planner_create (csrc/env.hpp). */
int qtos_env(const QtosPlanner *p, char *buf, int n);

/* Seconds spent in the KKT kernels / all kernels during the last qtos_plan_batch* call, from HIP
 * events on the launch stream (valid after the stream has been synchronised), and the number of
 * KKT launches.  Used by bench.py for the roofline figure. */
int qtos_last_timing(QtosPlanner *p, double *kkt_seconds, int *kkt_launches, double *total_seconds,
                     int *iterations);
/* Where the time of the last call went (same events, lane 0), seconds: out[0] first kernel -> end of the call, out[1] initial
 * guess, out[2] solve kernels, out[3] line-search / linearisation kernels with their counts, out[4] GAPS (a slot's last event
 * -> the next slot's first: the host reading the counts and launching; zero between slots queued at submit time), then counts:
 * out[5] launch slots with work, out[6] slots queued at submit time, out[7] launches that waited for the host, out[8] calls of
 * the handle that followed a launch pattern so far, out[9] of those, calls in which a problem sat a slot out.  n_out >= 10; with
 * n_out >= 14 also out[10] seconds / out[11] launches of the factorising kernel and out[12] / out[13] of k_chord (what
 * qtos_last_timing and qtos_last_timing_chord report: one call instead of three inside a timed loop). */
int qtos_last_timing_detail(QtosPlanner *p, double *out, int n_out);
/* The HIP events the three timing entry points read are recorded around every solve kernel and behind every launch slot of a
 * call (default on: bench.py's roofline figure is measured from them).  on = 0 keeps the call's first and last event only -- a
 * caller that does not read kernel times saves the event packets between its kernels; the timing entry points then return -1. */
int qtos_set_kernel_events(QtosPlanner *p, int on);
/* Per-solve report (the Ipopt log the reference's ./main prints: iteration table, final measures, evaluation counts).
 * on != 0: the calls submitted from now on record an iteration history per problem and, behind the call, evaluate the final
 * measures at the returned iterate (k_report, outside the launch pattern).  A call of one lane (B up to the GPU's compute
 * units) launches k_report behind its end event, so qtos_last_timing* do not count it; a call cut into lanes launches it
 * in front of the lanes' join, so its time enters total_seconds there.  k_report rewrites the problems' constraint values
 * and Jacobian in the workspace with those of the returned iterate: the qtos_debug_read_* readers see that linearisation
 * after a call with the report on.  The flag is latched per call at submit; returns -5 while a call is open (between
 * qtos_plan_submit and the end of qtos_plan_wait). */
int qtos_set_report(QtosPlanner *p, int on);

/* History record of one iteration (qtos_plan_report `rows`, QTOS_HIST_COLS doubles per row, row i = iteration i). */
#define QTOS_HIST_COLS 10
enum {
  QTOS_H_INF_PR = 0,  /* max violation of the working rows (qtos_debug_trace column 0)                     */
  QTOS_H_THETA,       /* max |c_i - s|, |c_e| (trace column 1)                                           */
  QTOS_H_MU,          /* barrier parameter after the step (trace column 3)                               */
  QTOS_H_DNORM,       /* max |dx| of the step's direction, node space (the step applied is alpha_pr times it) */
  QTOS_H_ALPHA_PR,    /* primal step length (trace column 2; 0 for a discarded chord step)               */
  QTOS_H_ALPHA_DU,    /* step length of the bound multipliers z (y comes whole from the KKT solve)       */
  QTOS_H_LS,          /* line-search trials (constraint evaluations) of the step; 0 in row 0             */
  QTOS_H_KIND,        /* 0 Newton step, 1 chord step, 2 discarded chord step                             */
  QTOS_H_COMPL,       /* max over inequality rows of |(s - l) z_l|, |(u - s) z_u|                        */
  QTOS_H_INF_DU       /* max |Je' y + Ji' (z_u - z_l)| over the KKT system's unknowns; in the
                         last row formed by k_report at the RETURNED iterate (for a stalled or failed problem the restored
                         best one, with the last iterate's s, z and y) while the row's other columns are the last iterate's */
};

/* Final report of problem b of the last call made with the report on. */
typedef struct QtosReport {
  int status;                  /* 0 converged, 1 out of iterations / stalled / jammed, 2 numerical failure       */
  int iterations;
  int n_rows;                  /* history rows: iterations + 1                                                    */
  int n_con_evals;             /* constraint evaluations: the starting point + every line-search trial            */
  int n_jac_evals;             /* Jacobian evaluations: the starting point + one per step the solve went on from  */
  int n_factorizations;        /* KKT solves with a fresh factorisation (Newton steps)                            */
  int n_chord_solves;          /* KKT solves with the stored factorisation (chord steps, discarded ones included) */
  int pad;
  double constraint_violation; /* at the returned iterate                                                         */
  double dual_infeasibility;
  double complementarity;
  double nlp_error;            /* max of the three (objective zero, Ipopt's scaling s_d = 1)                      */
} QtosReport;
/* Host pointers.  rows (may be null): up to max_rows history records of QTOS_HIST_COLS doubles.  Returns the number of
 * history rows (iterations + 1), -1 on bad arguments, -6 if the last call ran without the report or b is outside it. */
int qtos_plan_report(QtosPlanner *p, int b, QtosReport *out, double *rows, int max_rows);
/* Host-only: counts the Ipopt header prints that QtosDims lacks, from the host model of the full system (reduce_base = 0,
 * reduce_swing = 0): counts[0] / [1] structural nonzeros of the equality / inequality constraint Jacobian over the free
 * variables.  Returns the number written (min(n, 2)) or < 0. */
int qtos_analyze_counts(const QtosParams *params, long long *counts, int n);

/* The same for the chord-step launches (k_chord, QtosParams.chord_tol) of the last call. */
int qtos_last_timing_chord(QtosPlanner *p, double *chord_seconds, int *chord_launches);
/* Running totals over all qtos_plan_batch* calls of the handle since the last reset: problems returned with
 * status 0 and Newton iterations spent, tallied on the device at the end of every call (no read-back, no extra
 * work for the caller between batches).  Synchronises the stream of the last call.  reset != 0 clears them. */
int qtos_plan_totals(QtosPlanner *p, long long *converged, long long *iterations, int reset);

/* ---- introspection for the parity tests (host pointers) ------------------------------------ */
/* constraint values (B x n_cons) and, if J_out != NULL, the dense Jacobian (B x n_cons x n_vars,
 * columns of fixed variables zero, dropped rows zero) at the given nodes */
int qtos_debug_eval(QtosPlanner *p, int B, const double *start, const double *goal,
                    const int *map_id, const double *nodes, double *g_out, double *J_out);
/* one condensed KKT solve per problem with caller-supplied barrier weights:
 *   [delta I + Ji' diag(sig) Ji, Je'; Je, -eps I] [dx; y] = [-Ji' w; -g_e]
 * sig, w: B x n_cons (entries of inequality rows are used); dx_out: B x n_vars */
int qtos_debug_newton(QtosPlanner *p, int B, const double *start, const double *goal,
                      const int *map_id, const double *nodes, const double *sig, const double *w,
                      double *dx_out);
/* the same system once more through the chord-step kernel: the factorisation the preceding qtos_debug_newton
 * call left on the device + the right-hand side in elimination order (parity of k_chord with k_kkt2) */
int qtos_debug_chord(QtosPlanner *p, int B, double *dx_out);
/* QtosParams.reduce_base: a solve that is given nodes (`warm`) starts from their projection onto the space of the
 * B-spline coefficients (nodes of a C2 spline stay what they are; the reference's plans, whose acceleration continuity
 * holds to their CSV precision, move by that much).  This is that projection (host pointers, B x n_vars); without
 * reduce_base a copy. */
int qtos_project_nodes(QtosPlanner *p, int B, const double *nodes, double *nodes_out);
/* diagnostics (scratch/reduced_base_sweep.py, host-side emulations of the chain): the stage stream of problem b as the last
 * linearisation left it (qtos_debug_stream_len doubles), and the vector behind the last qtos_debug_residual call, by
 * POSITION of the elimination order: n_stages * pivots doubles (QtosDims) -- the positions count the dummy pivots that
 * fill short stages, QtosDims.n_unknowns does not */
int qtos_debug_stream_len(const QtosPlanner *p);
int qtos_debug_read_stream(QtosPlanner *p, int b, double *out);
int qtos_debug_read_rhs(QtosPlanner *p, int b, double *out);
/* a-posteriori residual of the system the preceding qtos_debug_newton call solved: res_rel_out[b] = max |b - K x| /
 * max |b|, K applied from the problem's stream without the factorisation (k_residual).  refine != 0: first one step of
 * iterative refinement through the stored factorisation (r = b - K x, K e = r by k_chord, x += e); dx_out (B x n_vars,
 * may be NULL): the (refined) solution.  SURVEY.md section 7-5: accuracy of the KKT solve vs a CPU factorisation. */
int qtos_debug_residual(QtosPlanner *p, int B, int refine, double *dx_out, double *res_rel_out);
/* working-set description: row_kind[n_cons] (0 dropped, 1 equality, 2 inequality), var_free[n_vars] (0/1), and the
 * elimination order BY POSITION: order[n_stages * pivots] (QtosDims) = var index, n_vars + row for a multiplier, or -1
 * for a dummy pivot (short stages, the fill of the last stage, the all-dummy stage pair mode may append): size the
 * buffer by n_stages * pivots, NOT by n_unknowns */
int qtos_debug_structure(const QtosPlanner *p, int *row_kind, int *var_free, int *order);
/* factor panels of problem b after the last KKT solve (n_stages x (front + 1) x 16 doubles: per stage
 * w = L^-T D^-1 y_F (16) then V = Y D^-1 L^-1 by front slot, column c of a row stored at
 * 4 (c & 3) + (c >> 2)) and the pivot slots (n_stages x 16) */
int qtos_debug_factor(QtosPlanner *p, int b, double *panel_out, int *piv_slot_out);
/* the starting point a solve without `warm` would use (straight-line guess or table guess), B x n_vars */
int qtos_debug_initial_guess(QtosPlanner *p, int B, const double *start, const double *goal,
                             const int *map_id, double *nodes_out);
/* per-iteration trace of the last plan call for problem b: rows of (viol, theta, alpha, mu),
 * at most max_iter rows; returns the number of rows */
int qtos_debug_trace(QtosPlanner *p, int b, double *trace_out);
/* final primal-dual state of problems 0 .. B-1 of the last plan call, by constraint row (n_cons doubles per problem and
 * array): slacks s, bound multipliers z_l, z_u (zero on rows that are not inequality rows of the working set) and the
 * equality multipliers y of the last KKT solve (zero for dropped rows and rows a reduction eliminated).  Any array may be
 * null. */
int qtos_debug_duals(QtosPlanner *p, int B, double *s, double *zl, double *zu, double *y);
/* What this build of the library contains: bit 0 is reserved and always 0 (it marked the experiment build of round 4, which
 * left the library; the other bits keep their numbers), bit 1 = per-wave cycle stamps (-DQTOS_STAMPS),
 * bit 2 = a development build with the benchmark's fronts only (-DQTOS_DEV_F128).  The product library returns 0. */
int qtos_build_flags(void);
/* The factor + solve kernel qtos_planner_create selected for this planner, e.g. "k_kkt2<128>", "k_kkt3<112, 1>",
 * "k_kkt5<128>" (the name rocprofv3 lists it under, without the namespace and the trailing template defaults): at most
 * n - 1 characters and a terminating zero into buf; returns the length of the full name.
 * Selection (environment variable QTOS_KKT, read at creation): unset = k_kkt3 MODE 1 for fronts of at most 112 slots,
 * k_kkt2 above; 2 = k_kkt2; 4 = k_kkt3 MODE 1 (fronts up to 128); 6 = k_kkt5 -- two 16-pivot stages per set of barriers,
 * pair-mode analysis (fronts 96 .. 144 without continuation records; otherwise the default).  Every choice solves the same
 * KKT systems; plans of different kernels differ by rounding (2e-8 on the walk, up to 5e-6 on the trot). */
int qtos_kkt_kernel(const QtosPlanner *p, char *buf, int n);
/* Host-only: the name qtos_kkt_kernel would report for a planner of these parameters created now, under the environment as
 * it is now (the same choice, no GPU needed); returns the length of the full name, < 0 where qtos_planner_create would fail
 * in the analysis. */
int qtos_analyze_kernel(const QtosParams *params, char *buf, int n);

/* ---- self-test of the elimination order ------------------------------------------------------
 * The factor + solve kernels eliminate the KKT matrix WITHOUT pivoting, in an order the host analysis picks from time keys
 * (QtosDims.order_rule).  Whether that order is sound for a transcription shows in one KKT solve with barrier weights over six
 * decades: its residual, and the size of the factor's entries (1 / eps_dual is the norm; an order that loses digits has entries
 * tens of times larger).  The interior-point loop absorbs a bad solve -- plans still come back with status 0 --, so the check
 * has to be made on purpose. */
typedef struct QtosSelftest {
  int order_rule, front, n_stages;  /* of the planner that was tested                              */
  int n_problems;                   /* systems solved (2)                                          */
  int worst_stage;                  /* stage that holds max_factor                                 */
  int passed;                       /* residual <= tol_residual && max_factor <= growth_limit      */
  double residual;                  /* max over the systems of max|b - K x| / max|b|               */
  double residual_refined;          /* the same behind one step of refinement through k_chord;
                                       -1 where the planner has no chord kernel                    */
  double max_factor;                /* largest |entry| of the factor panels' V part                */
  double growth_limit;              /* 1.05 / eps_dual                                             */
  double tol_residual;              /* as passed in (<= 0: 1e-6)                                   */
  double seconds;                   /* wall time of the self-test, host clock                      */
} QtosSelftest;
/* Two KKT systems on the planner's own device through the planner's own factor + solve and chord kernels: flat ground (the
 * handle's heightfields and table of nominal plans are ignored, and stay), the rest start at the origin in nominal stance, the
 * goal 0.09 m per second of horizon straight ahead (qtos_selftest_problem), towr's straight-line guess + dx0, barrier weights
 * sig and right-hand sides w of qtos_selftest_inputs(seed, problem 0 / 1).  One solve, its residual (k_residual: K applied
 * without the factorisation), one step of refinement as qtos_debug_residual(refine = 1), and a reduction over the factor panels
 * on the device (k_panel_absmax).  Returns 0 with `out` filled -- pass or fail is out->passed, not the return code --, -1 bad
 * arguments, -2 HIP error, -5 while a call is open.  Uses the workspace of the qtos_debug_* entry points; launch pattern, totals,
 * report flag and heightfields of the handle stay as they were: a plan call behind it returns the bits it would have returned
 * without it. */
int qtos_planner_selftest(QtosPlanner *p, unsigned long long seed, double tol_residual, QtosSelftest *out);
/* Host-only: the self-test's random inputs for problem b (dx0: n_vars; sig, w: n_cons doubles, sizes from qtos_analyze) -- the
 * very function the self-test calls.  Counter-based, no state:
 *   mix(z)     z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB;
 *              z ^ z >> 31                                                   (splitmix64; 64-bit wrap-around arithmetic)
 *   bits(a, i) mix(mix(mix(mix(seed) ^ b) ^ a) ^ i)                          (qtos_selftest_bits; array a: 0 dx0, 1 sig, 2 w)
 *   u(a, i)    ((bits(a, i) >> 11) + 0.5) * 2^-53                            in (0, 1)
 *   n(a, i)    sqrt(-2 log u(a, 2 i)) * cos(2 pi u(a, 2 i + 1))              Box-Muller, one normal per pair; 2 pi = 6.283185307179586
 *   dx0[i] = 0.01 n(0, i)     sig[r] = pow(10, -3 + 6 u(1, r))     w[r] = n(2, r) * sqrt(sig[r])
 * in IEEE double with the host's libm.  Returns 0, -1 bad arguments / parameters. */
int qtos_selftest_inputs(const QtosParams *params, unsigned long long seed, int b, double *dx0, double *sig, double *w);
unsigned long long qtos_selftest_bits(unsigned long long seed, int problem, int array, unsigned long long index);
/* Host-only: start (24 doubles) and goal (3) of the self-test's problems (both problems have the same). */
int qtos_selftest_problem(const QtosParams *params, double *start, double *goal);
/* qtos_planner_create with the self-test as a gate.  Candidates: with QTOS_ORDER set, that rule alone.  Otherwise the rules in
 * rules_mask (bit r = rule r; 0 = what the automatic choice considers: rules 2 and 1 on a reduced base, rule 0 where the base
 * is not reduced -- there rule 0 is the only candidate whatever the mask), sorted by the preference of the automatic choice:
 * smaller front, fewer stages, no continuation records, then 2 before 1 before 0.  With rules_mask = 0 the first candidate is
 * the planner qtos_planner_create builds.  Each candidate is built and tested (seed 0, tol_residual as above); the first that
 * passes is returned, the others are destroyed.  tried[i] (up to max_tried; *n_tried of them written) records every attempt
 * in order; a candidate whose analysis or creation fails is recorded with passed = 0, front = 0 and skipped.
 * Returns 0 and the planner; -6 and *out = NULL if no candidate passes (stderr names rule, residual, growth and worst stage
 * of each attempt); -1 .. -4 as qtos_planner_create when nothing could be built; -2 before any analysis without a device. */
int qtos_planner_create_checked(const QtosParams *params, int max_batch, int device, int rules_mask, double tol_residual,
                                QtosPlanner **out, QtosSelftest *tried, int max_tried, int *n_tried);
/* Host-only: the candidates in the order qtos_planner_create_checked would try them under the environment as it is now (rule,
 * front and stages of each into the arrays, up to n; any may be NULL); returns the count. */
int qtos_analyze_candidates(const QtosParams *params, int rules_mask, int *rules, int *fronts, int *stages, int n);

#ifdef __cplusplus
}
#endif
#endif
