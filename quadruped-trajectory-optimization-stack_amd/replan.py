"""Receding-horizon re-planning: counterpart of the reference's planning thread.

``ReplanLoop`` mirrors ``scripts/main.py``: ``_run`` (26-103: first plan from the rest pose toward
``spine_step``, then the update thread) and ``_update`` (26-62), whose loop alternates three states

    plan     ``Combiner.plan``: hand-over state = the row ``lookahead`` steps ahead of the robot's clock in the
             plan being executed, advanced until every foot stands on a known terrain height
             (QTOS/combiner.py:158-179, 245-296); goal = ``Global_Planner.pop()`` (LIFO,
             QTOS/planner.py:232-239); one solver call
    wait     until the consumer has eaten ``f_steps`` rows of the current plan (scripts/main.py:52)
    stitch   ``Combiner.combine``: old[cutoff-1 : next_traj_step] ++ new (QTOS/combiner.py:125-135), after
             which the consumer restarts its row counter (scripts/run.py:177-183)

and stops when the start of the last plan is within 0.1 m of its goal (scripts/main.py:40-46).  The
solver call is ``LocalPlanner.solve_batch`` (one GPU solve) instead of ``docker exec ./main``; the
consumer is whoever calls ``tick(step, runtime)`` with the reference's two counters (``RUN.step``,
``ROBOT_CFG.runtime``) -- ``run()`` drives it with a consumer that tracks the plan perfectly.

``ShiftedWindows`` is the batched form used for BASELINE configs[4]: many independent robots (windows) on one
GPU, every step = one replan of every window with the hand-over semantics above.

Starting point of a replan.  ``qtos_shift_warm`` builds the time-shifted previous plan and both
classes can use it (``shifted_warm_start=True`` / ``warm="shifted"``), but it is NOT the default: the reference
restarts its gait schedule with every plan, so the previous plan read 2.5 s later lifts other feet at other times
than the new schedule, and measured on the randomized heightfields (scratch/shift_exp.py, 64 windows x 6 replans,
200-knot plans) the shifted plan needs 4.8-5.6 Newton iterations (slowest window 9-16) against 4.1-4.2 (slowest 5-6)
from towr's straight-line guess, whatever the slack push and whichever variable sets are shifted.  A batch waits
for its slowest window, so the loops start cold, like the reference's solver.
"""
import ctypes as C

import numpy as np

from . import capi, flags
from .capi import ptr
from .stitcher import Stitcher, row_state


class ReplanLoop:
    def __init__(self, local_planner, global_planner, args, lookahead=3750, f_steps=2500, hz=1000,
                 height_set=(0.0,), mode="reference", shifted_warm_start=False):
        self.lp, self.gp = local_planner, global_planner
        self.args = dict(args)
        self.f_steps, self.hz = int(f_steps), hz
        self.st = Stitcher(lookahead=lookahead, hz=hz, height_set=height_set, mode=mode)
        self.shifted = shifted_warm_start
        self.plan = None          # rows of the plan being executed (the reference's ./data/traj/towr.csv)
        self.new = None           # rows of the plan waiting to be stitched (/tmp/towr.csv)
        self.nodes = None         # nodes of the newest plan and the time stamp of its first row
        self.nodes_t0 = 0.0
        self._wait = False
        self.done = False
        self.goal_diff = np.inf
        self.events = []          # (event, runtime) log: "plan", "stitch", "done"
        self.statuses = []

    # scripts/main.py:81-92 + Combiner.plan_init (QTOS/combiner.py:137-156)
    def start(self):
        a = self.args
        a['-s'], a['-s_ang'] = [0, 0, 0.24], [0, 0, 0]
        a['-e1'], a['-e2'] = [0.21, 0.19, 0.0], [0.21, -0.19, 0.0]
        a['-e3'], a['-e4'] = [-0.21, 0.19, 0.0], [-0.21, -0.19, 0.0]
        a['-g'] = [float(v) for v in self.gp.spine_step(np.array(a['-s'], float), 0.0)]
        status = self.lp.solve_batch([a])[0]
        self.statuses.append(status)
        if status != 0:
            raise RuntimeError("first plan failed (the reference exits here: scripts/main.py:101-103)")
        self.plan = np.array(self.lp.last["rows"][0])
        self.nodes, self.nodes_t0 = np.array(self.lp.last["nodes"][0]), 0.0
        self.events.append(("plan", 0.0))
        return status

    # one pass of the loop body of _update (scripts/main.py:34-62) with the consumer's counters
    def tick(self, step, runtime):
        if self.done:
            return "done"
        self.st.cutoff_idx = int(step)
        last_t = round(runtime, 3)
        self.goal_diff = float(np.linalg.norm(np.array(self.args['-s'])[0:2] - np.array(self.args['-g'])[0:2]))
        self.gp.update(last_t)
        if self.gp.max_t < last_t - 5.0:            # QTOS/combiner.py:224-226
            self.done = True
        if self.goal_diff < 0.1 or self.done:
            self.done = True
            self.events.append(("done", runtime))
            return "done"
        if not self._wait:
            state = self.st.state(np.round(self.plan, 6), last_t)     # the CSV carries 6 digits
            if not self.gp.empty():
                _, goal = self.gp.pop()
                goal = [float(v) for v in goal]
            else:                                                       # Combiner._step (QTOS/combiner.py:229-238)
                pos = np.array(state["CoM"])
                d = np.clip(np.array(self.gp.robot_goal) - pos, -self.gp.step_size, self.gp.step_size)
                goal = [float(pos[0] + d[0]), float(pos[1] + d[1]), 0.24]
            self.args = self.st.plan_args(self.args, state, runtime, goal)
            warm = None
            if self.shifted and self.nodes is not None:
                s, g, t0 = flags.problem_arrays(self.args)
                off = max(self.args['-t'] - self.nodes_t0, 0.0)
                warm = self.lp.planner(self.args.get('-duration')).shift_warm(self.nodes[None], off, np.array(s)[None], np.array(g)[None])
            self.statuses.append(self.lp.solve_batch([self.args], warm=warm)[0])   # (the reference ignores this status: scripts/main.py:50)
            self.new = np.array(self.lp.last["rows"][0])
            self.nodes, self.nodes_t0 = np.array(self.lp.last["nodes"][0]), float(self.args['-t'])
            self._wait = True
            self.events.append(("plan", runtime))
            return "plan"
        if self.st.cutoff_idx >= self.f_steps:
            self.plan = self.st.combine(self.plan, self.new)
            self._wait = False
            self.events.append(("stitch", runtime))
            return "stitch"       # the consumer re-opens the plan: its row counter restarts at 0
        return None

    def run(self, max_plans=8, dt_tick=0.05):
        """Drive the loop with a consumer that follows the plan exactly: one row per millisecond."""
        self.start()
        step, runtime = 0, 0.0
        while not self.done and sum(1 for e in self.events if e[0] == "plan") < max_plans:
            ev = self.tick(step, runtime)
            if ev == "stitch":
                step = 0
            adv = int(round(dt_tick * self.hz))
            step += adv
            runtime += adv / self.hz
        return self.plan


def handover_index(rows, k0, n_search, rule, heights=(0.0,)):
    """The hand-over rule of k_handover (qtos_handover*) stated in numpy, on a sampled row table: the first of the rows
    k0 .. k0 + n_search (inclusive; as far as the table goes) that passes the contact rule, k0 where none does.

    rule 0   force rule: f_z > 0 for all four feet (columns 27, 30, 33, 36)
    rule 1   height-set rule (Combiner._state, QTOS/combiner.py:78-92; ``Stitcher.legs_in_contact``): every foot's z
             (columns 9, 12, 15, 18) at 6 decimals is one of ``heights``: rint(z * 1e6) == rint(h * 1e6)

    rows: (n_rows, 37) -> int, or (B, n_rows, 37) -> int64 array.  The table must be sampled from row 0 at the rate the
    kernel is given (a table that covers the whole plan holds every row the kernel can pick: later rows repeat the last)."""
    rows = np.asarray(rows, np.float64)
    if rows.ndim == 2:
        return int(handover_index(rows[None], k0, n_search, rule, heights)[0])
    k0, n_search = int(k0), int(n_search)
    cand = rows[:, k0:k0 + n_search + 1, :]
    if rule == 0:
        ok = (cand[:, :, 27:37:3] > 0).all(axis=2)
    elif rule == 1:
        known = np.rint(np.asarray([float(h) for h in heights], np.float64) * 1e6)
        ok = (np.rint(cand[:, :, 9:19:3] * 1e6)[..., None] == known).any(axis=3).all(axis=2)
    else:
        raise ValueError("rule 0 (force) or 1 (height set)")
    return np.where(ok.any(axis=1), k0 + ok.argmax(axis=1), k0).astype(np.int64)


class ShiftedWindows:
    """B independent receding windows on one planner: every ``replan()`` starts every window from the row
    ``advance`` seconds into its newest plan (= the reference's hand-over row: a new plan starts ``lookahead``
    rows ahead of the robot's clock and the next one is asked for ``f_steps`` rows later, i.e. ``f_steps`` rows
    into the newest plan), moved on until all four feet are in contact; goals move with the windows; the
    previous plan shifted by that time is the warm start.  Everything stays on the device (torch tensors).

    handover   "kernel": one launch of k_handover per replan picks every window's row and writes start / offset / goal
               (qtos_handover_device; the default where the library has it); "rows": the whole row table is sampled
               (qtos_sample_csv_device) and searched with torch ops -- the same bits, kept for A/B
    contact    "force" (all four f_z > 0) or "heights" (the reference's rule: every foot's z at 6 decimals in
               ``height_set``, Combiner._state; "kernel" only).  They differ at stance boundaries, where the force spline
               is exactly zero (``handover_index``).
    trajectory None (the default): nothing is kept of the plans but the newest.  An int: every window keeps a ring of that many
               CSV rows (``self.traj``, B x trajectory x 37, with the running row count ``self.cursor``) and every replan
               appends the rows the window executed of the plan it hands over from (k_stitch through qtos_stitch_device,
               ``stitcher.stitch_segments``); ``self.t0`` is then the windows' clock: the time stamp of row 0 of the newest
               plan.  ``finish()`` appends the rest of the newest plan, ``trajectory_rows(b)`` reads a window's ring.
    stitch     "clean" (every row: old[:r] ++ new) or "reference" (the reference's files, whose first row pd.read_csv eats:
               old[1:][:r] ++ new[1:], ``Stitcher(mode="reference")``)
    path       None (the default): every goal moves by ``goal_step`` per plan.  A dict: the goals come from the windows' global
               paths, as the reference's come from its global planner (k_path_goal through qtos_path_goal_device, the rule:
               ``global_planner.path_goal``) -- ``table`` (``global_planner.path_table``), ``step_size``, and optionally
               ``path_id`` (B; default window b follows path b), ``map_yx`` (n_maps x rows x cols height grids, row = y) with
               its own ``map_id`` (B; default map 0), ``cell`` (0.1), ``origin`` ((1.0, 1.0)), ``horizon`` (the plans'
               duration), ``tol`` (1e-5), ``z_offset`` (0.24), ``stop_dist`` (0: no bit 1), ``clamp_x`` (False).  The table and
               the grids are uploaded once, here.  ``goal_step`` may then be None.  The first plan's goal is the step from the
               start state at clock 0 (plan_init); every later one follows the hand-over on the same stream, with its start and
               offset.  ``self.clock`` (B, f64: the plan time of row 0 of the newest plan) and ``self.done`` (B, int32: bit 0
               the path's end lies 5 s + ``advance`` behind the plan's start, bit 1 the goal is within ``stop_dist``) live on
               the device; ``self.path_params_init`` / ``self.path_params`` are the QtosPathGoal of the first / later calls.
               Instead of ``table``, ``plan`` = dict(``bool_map`` n_maps x rows x cols or rows x cols, ``robot_goal`` B x 3, and
               optionally ``map_id`` (B; default map 0), ``max_cells``, ``max_pieces``, ``max_open`` (4096), ``height_bound``
               (0.2)) plans the paths on the device (k_path_plan through qtos_path_plan_device, the rule:
               ``global_planner.path_plan``): window b follows its own path from ``start[b, 0:2]`` to ``robot_goal[b]``.
               ``self.path_status`` (B, int32; 0 found), ``self.path_cells`` and ``self.path_n_cells`` live on the device, a
               window without a path has bit 2 of ``self.done`` set, and ``repath()`` plans the paths anew.
    path_base  "spine" (Global_Planner.update: the step is taken from the spine at the plan's start) or "state" (from the state
               the plan starts from), for every plan but the first
    path_hold  True: a window whose done bits are set stands still (its goal is its start) instead of following the spline's
               extrapolation beyond the path's end
    joints     None (the default): nothing is queued.  A dict (needs ``trajectory``): every window also keeps a ring of joint rows
               (``self.joint_traj``, B x trajectory x 37: time stamp, q, qdot, tau of the twelve joints) and their status words
               (``self.joint_status``, B x trajectory), filled row for row with ``self.traj`` by k_joint_rows
               (qtos_joint_rows_device, the rule: ``joints.joint_rows``), queued in front of every stitch and in ``finish()``.  The
               dict's entries are ``capi.joint_params``' keywords (ee_shift, kp, kd, hip_scale, knee_scale, ankle_scale, tau_max,
               feed_forward, robot); ``joint_rows(b)`` reads a window's ring.
    track      None (the default): nothing is queued and nothing is allocated.  A dict (needs ``trajectory``): every window also
               keeps a ring of measured states (``self.meas_traj``, B x trajectory x 18, or x 19 with ``quaternion``: the caller's to
               fill, at ring rows (cursor + j) mod trajectory, for the rows a plan executes before the next takes over), a ring of
               track rows (``self.track_traj``, B x trajectory x 26: time stamp, measured pose, five errors, two running totals),
               their status words (``self.track_status``) and the accumulators ``self.track_count`` (B x 2, int64: calls, recorded)
               and ``self.track_total`` (B x 2: total_com, total_feet), filled by k_track (qtos_track_device, the rule:
               ``tracking.track_rows``), queued in front of every stitch and in ``finish()``, behind the joint rows where both are
               on.  The dict's entries are ``capi.track_params``' keywords (ee_shift, delay, rule, quaternion, robot), ``goal_x`` (a
               number or one per window: status bit 1 of a row whose measured CoM x has reached it) and ``fill`` (a callable
               taking the windows, called on the set's stream in front of every track call: the last place to write
               ``meas_traj``, e.g. from the joint ring just filled); ``track_rows(b)`` reads a window's ring.
    feedback   None (the default): every plan starts from the old plan's own hand-over row, nothing is queued and nothing is
               allocated.  A dict (needs ``track``, whose measured ring it reads): behind every hand-over the start vectors are
               corrected by the tracking error at the hand-over row (k_start_feedback through qtos_start_feedback_device, the rule:
               ``feedback.start_feedback``), in place on ``self.start`` and, without a path, ``self.goal``;
               ``self.feedback_status`` (B, int32: bit 0 corrected, 1 clipped, 2 gimbal, 3 fell back, 5 no measurement, 6 + f foot
               f snapped by more than snap_tol) and ``self.feedback_err`` (B x 18: the clipped error) live on the device.  The
               dict's entries are ``capi.feedback_params``' keywords (gain_pos, gain_ang, gain_foot, max_pos, max_ang, max_foot,
               latency, snap, zero_filter, rom_tol, snap_tol, nominal, max_deviation, cfg; the leg and the quaternion flag are the
               track's).  The order of a replan is then hand-over, joint rows, track (whose ``fill`` writes the measurements of the
               segment), feedback, path goal (so that ``path_base="state"`` sees the corrected start), stitch.
    rollout    None (the default): nothing is queued and nothing is allocated, and ``meas_traj`` is the caller's to fill.  A dict
               (needs ``track``, whose ``meas_traj`` it fills): the windows' robots are simulated rigid bodies (k_rollout through
               qtos_rollout_device, the rule: ``rollout.rollout_rows``), queued behind the joint rows and in front of the track
               call, and in ``finish()``, over exactly the rows the stitch appends and with its cursor.  A window's first call
               with rows sets its body on its plan (QTOS_ROLLOUT_PENDING in its word, spent per window, as QTOS_ROLLOUT_INIT sets
               it); every later one goes on from the carried state, so the body does
               not jump when the plan under it changes.  ``self.rollout_state`` (B x 13), ``self.rollout_count`` and
               ``self.rollout_word`` (B) and the rows' status words ``self.rollout_status`` (B x trajectory) live on the device.
               The dict's entries are ``capi.rollout_params``' keywords (substeps, ff_scale, the gains and limits, dev_max,
               tilt_max, push_from, push_ticks, mass, gravity, inertia_b, cfg; the quaternion flag is the track's),
               ``mass_scale`` (a number or one per window), ``push`` (B x 6) and ``rows=True`` to keep ``self.rollout_traj`` (B x
               trajectory x 20); ``rollout_rows(b)`` reads a window's ring.  With ``joints`` on the measured joint angles are the
               commanded ones; without, those twelve columns of ``meas_traj`` are not touched.  A ``fill`` callable of ``track``
               still runs, behind the rollout: the place to add sensor noise.  The planner's reference-compat inertia tensor is
               indefinite: with gains, give ``inertia_b=config.INERTIA_PHYSICAL``.  An entry ``feet=dict(arm=, damping=, w_min=,
               mu=, f_max=, limit=)`` (``capi.rollout_feet_params``' keywords; arm, damping and w_min default to the fit's, mu and
               f_max to the configuration's friction and force limit) queues k_rollout_feet (qtos_rollout_feet_device, the rule:
               ``rollout_feet.rollout_feet_rows``) IN PLACE of k_rollout, at the same point and with the same carried arrays: the
               feedback wrench is delivered through the stance feet, optionally limited to what a foot can do, and
               ``self.rollout_feet_traj`` (B x trajectory x 16: applied forces, what the feet did not deliver) is filled beside the
               other rings; ``rollout_feet_rows(b)`` reads a window's.  Without ``feet`` nothing of it is allocated or queued.
               ``feet=dict(..., limit="qp", mu_end=, act_tol=, max_iter=)`` (``capi.rollout_qp_params``' keywords) queues
               k_rollout_qp (qtos_rollout_qp_device, the rule: ``rollout_qp.rollout_qp_rows``) in place of k_rollout_feet, with the
               same carried arrays: every step's stance forces are the fit's where those obey the limits and the pyramid QP's
               where they do not; ``self.rollout_qp_traj`` (B x trajectory x 8, the solve's columns of every tick's first step) is
               filled as well, and ``rollout_qp_rows(b)`` reads a window's.  ``limit=True / False`` queue and allocate what they
               did without it.
    check      None (the default): nothing is queued and nothing is allocated.  A ``capi.check_params(...)`` (needs
               ``trajectory``; its tol is read, its rate and rows are the stitch's): k_plan_check (qtos_plan_check_device, the
               rule: ``plan_check.check_rows`` / ``summarise`` / ``accumulate``) is queued in front of every stitch and in
               ``finish()``, over exactly the rows that stitch appends and with its cursor, and merges what they violate into
               ``self.check_summary`` (B x 5 records as B x 5 x 3 words); ``check_worst()`` reads them.  It writes nothing else:
               plans and trajectory rows are the same bits with and without it.
    fit        None (the default): nothing is queued and nothing is allocated.  A dict of ``capi.fit_params``' keywords (arm, damping,
               w_min, excess_tol, tol, robot, ee_shift; needs ``trajectory``) and ``mass_scale`` (a number or one per window), or a
               ``capi.fit_params(...)`` whose rate and rows become the stitch's: k_force_fit (qtos_force_fit_device, the rule:
               ``force_fit.fit_rows`` / ``summarise`` / ``accumulate``) is queued behind the joint rows and in front of every stitch
               and in ``finish()``, over exactly the rows that stitch appends and with its cursor.  It fills a ring next to the joint
               ring (``self.fit_traj``, B x trajectory x 32: time stamp, fitted forces, residual rows, change, feed-forward torques
               at the joint ring's angles -- without ``joints`` those twelve columns stay zero) with its status words
               (``self.fit_status``) and merges the four families into ``self.fit_summary`` (B x 4 records as B x 4 x 3 words);
               ``fit_rows(b)`` and ``fit_worst()`` read them.  With ``limits=dict(mu=, f_max=, mu_end=, act_tol=, max_iter=)`` among
               the keywords (or a ``capi.qp_params(...)``) k_force_qp (qtos_force_qp_device, the rule: ``force_qp.qp_rows``) is
               queued in that place instead: the fit inside the friction pyramid, into the same fit ring and a ring of the solve's
               eight columns (``self.qp_traj``, read by ``qp_rows(b)``); the fourth family is then ``limited``.  Plans, trajectory rows and joint rows are the same bits with and
               without it."""

    def __init__(self, planner, start, goal_step, map_id=None, advance=2.5, search=0.4, stream=None, warm="none", x_range=None,
                 handover=None, contact="force", height_set=(0.0,), trajectory=None, stitch="clean", path=None, path_base="spine",
                 path_hold=True, joints=None, track=None, feedback=None, check=None, rollout=None, fit=None):
        import torch
        self.torch = torch
        self.P = planner
        dev = torch.device("cuda", planner.device if hasattr(planner, "device") else 0)
        self.dev = dev
        B = len(start)
        self.B = B
        f64 = dict(dtype=torch.float64, device=dev)
        self.start = torch.as_tensor(np.asarray(start), **f64).contiguous()
        self.path = path
        if path is None:
            self.goal_step = torch.as_tensor(np.asarray(goal_step), **f64).contiguous()     # (B, 3): per-plan displacement
            self.goal = self.start[:, 0:3] + self.goal_step
            self.goal[:, 2] = 0.24
            self.goal = self.goal.contiguous()
        else:
            self.goal_step = None
            self.goal = torch.zeros((B, 3), **f64)       # (written by k_path_goal in front of every plan, the first included)
            self._init_path(path, path_base, path_hold, float(advance))
        self.map_id = None if map_id is None else torch.as_tensor(np.asarray(map_id), dtype=torch.int32, device=dev).contiguous()
        self.nodes = torch.empty((B, planner.n), **f64)
        self.prev = torch.empty((B, planner.n), **f64)
        self.warm = torch.empty((B, planner.n), **f64)
        self.status = torch.empty((B,), dtype=torch.int32, device=dev)
        self.iters = torch.empty((B,), dtype=torch.int32, device=dev)
        self.viol = torch.empty((B,), **f64)
        self.advance, self.hz = float(advance), 1000.0
        self.n_search = int(round(search * self.hz))
        if handover is None:
            handover = "kernel" if planner.has("qtos_handover_device") else "rows"
        if handover not in ("kernel", "rows") or contact not in ("force", "heights"):
            raise ValueError("handover is 'kernel' or 'rows', contact 'force' or 'heights'")
        if contact == "heights" and handover != "kernel":
            raise ValueError("contact='heights' needs handover='kernel'")
        if handover == "kernel":
            planner._need("qtos_handover_device", "hand-over kernel")
        self.handover, self.contact = handover, contact
        k0 = int(round(advance * self.hz))
        if handover == "rows":
            self.rows = torch.empty((B, k0 + self.n_search + 1, 37), **f64)
        else:
            # (the row counts are rounded here, once: the kernel gets times that round to exactly these rows)
            self._hand = capi.handover_params(k0 / self.hz, self.n_search / self.hz, self.hz, contact, height_set, False, x_range)
            self.row = torch.zeros((B,), dtype=torch.int32, device=dev)      # hand-over row of the last replan
        self.t0 = torch.zeros((B,), **f64)
        self.offset = torch.zeros((B,), **f64)
        self.traj = None
        if trajectory is not None:
            if stitch not in capi.STITCH_MODES:
                raise ValueError("stitch is 'clean' or 'reference'")
            planner._need("qtos_stitch_device", "stitch kernel")
            self._stitch = capi.stitch_params(int(trajectory), stitch, 0, self.hz, True)
            self.traj = torch.zeros((B, int(trajectory), 37), **f64)
            self.cursor = torch.zeros((B,), dtype=torch.int64, device=dev)
            if handover == "rows":
                self.row = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.joint_traj = None
        if joints is not None:
            if self.traj is None:
                raise ValueError("joints needs a trajectory ring (trajectory=N)")
            planner._need("qtos_joint_rows_device", "joint-rows kernel")
            self._joint = capi.joint_params(hz=self.hz, first_row=int(self._stitch.first_row), capacity=int(trajectory), **dict(joints))
            self.joint_traj = torch.zeros((B, int(trajectory), 37), **f64)
            self.joint_status = torch.zeros((B, int(trajectory)), dtype=torch.int32, device=dev)
        self.track_traj = None
        if track is not None:
            if self.traj is None:
                raise ValueError("track needs a trajectory ring (trajectory=N)")
            planner._need("qtos_track_device", "track kernel")
            track = dict(track)
            goal_x, self._track_fill = track.pop("goal_x", None), track.pop("fill", None)
            self._track = capi.track_params(hz=self.hz, first_row=int(self._stitch.first_row), capacity=int(trajectory), **track)
            self.meas_traj = torch.zeros((B, int(trajectory), 19 if self._track.flags & capi.TRACK_QUAT else 18), **f64)
            self.track_traj = torch.zeros((B, int(trajectory), capi.TRACK_COLS), **f64)
            self.track_status = torch.zeros((B, int(trajectory)), dtype=torch.int32, device=dev)
            self.track_count = torch.zeros((B, 2), dtype=torch.int64, device=dev)
            self.track_total = torch.zeros((B, 2), **f64)
            self.track_goal_x = None
            if goal_x is not None:
                self.track_goal_x = torch.as_tensor(np.broadcast_to(np.asarray(goal_x, np.float64), (B,)).copy(), **f64)
        self._rollout = None
        if rollout is not None:
            if self.track_traj is None:
                raise ValueError("rollout needs the measured ring of track (track=dict(...)), which it fills")
            planner._need("qtos_rollout_device", "rollout kernel")
            kw = dict(rollout)
            scale, push, keep = kw.pop("mass_scale", None), kw.pop("push", None), kw.pop("rows", False)
            feet = kw.pop("feet", None)
            kw.setdefault("cfg", getattr(planner, "cfg", None))
            self._rollout = capi.rollout_params(hz=self.hz, first_row=int(self._stitch.first_row), capacity=int(trajectory),
                                                quaternion=bool(self._track.flags & capi.TRACK_QUAT), **kw)
            self.rollout_state = torch.zeros((B, capi.ROLLOUT_STATE), **f64)
            self.rollout_count = torch.zeros((B,), dtype=torch.int64, device=dev)
            self.rollout_word = torch.full((B,), capi.ROLLOUT_PENDING, dtype=torch.int32, device=dev)
            self.rollout_status = torch.zeros((B, int(trajectory)), dtype=torch.int32, device=dev)
            self.rollout_traj = torch.zeros((B, int(trajectory), capi.ROLLOUT_COLS), **f64) if keep else None
            up = lambda a, shape: None if a is None else torch.as_tensor(np.broadcast_to(np.asarray(a, np.float64), shape).copy(), **f64)
            self._rollout_scale, self._rollout_push = up(scale, (B,)), up(push, (B, 6))
            self._feet, self._feet_qp = None, False
            if feet is not None:
                planner._need("qtos_rollout_feet_device", "feet rollout kernel")
                fk = dict(feet)
                fk.setdefault("cfg", kw["cfg"])
                self._feet_qp = fk.get("limit") == "qp"
                if self._feet_qp:                                            # (k_rollout_qp in place of k_rollout_feet)
                    planner._need("qtos_rollout_qp_device", "QP rollout kernel")
                    del fk["limit"]
                    self._feet = capi.rollout_qp_params(**fk)
                    self.rollout_qp_traj = torch.zeros((B, int(trajectory), capi.ROLLOUT_QP_COLS), **f64)
                else:
                    self._feet = capi.rollout_feet_params(**fk)              # (its body is the call's QtosRollout, put in by _rollout_rows)
                self.rollout_feet_traj = torch.zeros((B, int(trajectory), capi.ROLLOUT_FEET_COLS), **f64)
        self._feedback = None
        if feedback is not None:
            if self.track_traj is None:
                raise ValueError("feedback needs the measured ring of track (track=dict(...))")
            planner._need("qtos_start_feedback_device", "feedback hand-over")
            kw = dict(feedback)
            kw.setdefault("cfg", getattr(planner, "cfg", None))
            t = self._track
            self._feedback = capi.feedback_params(hz=self.hz, first_row=int(self._stitch.first_row), capacity=int(trajectory),
                                                  quaternion=bool(t.flags & capi.TRACK_QUAT), ee_shift=float(t.ee_shift), robot=t, **kw)
            self.feedback_status = torch.zeros((B,), dtype=torch.int32, device=dev)
            self.feedback_err = torch.zeros((B, 18), **f64)
        self._check = None
        if check is not None:
            from . import plan_check
            if self.traj is None:
                raise ValueError("check needs a trajectory ring (trajectory=N)")
            planner._need("qtos_plan_check_device", "plan-check kernel")
            # the stitch's rows: its first row, its clamp of the count (the ring's capacity), its clock
            self._check = check.copy()
            self._check.hz, self._check.first_row, self._check.n_rows = self.hz, int(self._stitch.first_row), int(trajectory)
            self._check.flags |= capi.CHECK_ACCUMULATE
            self.check_summary = torch.from_numpy(plan_check.empty_summary(B).view(np.float64).reshape(B, 5, 3).copy()).to(dev)
        self._fit = None
        if fit is not None:
            from . import force_fit
            if self.traj is None:
                raise ValueError("fit needs a trajectory ring (trajectory=N)")
            planner._need("qtos_force_fit_device", "force-fit kernel")
            scale, limits = None, None
            if isinstance(fit, (capi.QtosForceFit, capi.QtosForceQp)):
                self._fit = fit.copy()
                limits = isinstance(fit, capi.QtosForceQp) or None
            else:
                kw = dict(fit)
                scale, limits = kw.pop("mass_scale", None), kw.pop("limits", None)
                if limits is None:
                    self._fit = capi.fit_params(kw.pop("cfg", getattr(planner, "cfg", None)), **kw)
                else:
                    self._fit = capi.qp_params(kw.pop("cfg", getattr(planner, "cfg", None)), **kw, **dict(limits))
            if limits is not None:                    # the fit inside the friction pyramid: k_force_qp in k_force_fit's place
                planner._need("qtos_force_qp_device", "force-QP kernel")
                self.qp_traj = torch.zeros((B, int(trajectory), capi.QP_COLS), **f64)
            # the stitch's rows: its first row, its ring, its clock
            self._fit.hz, self._fit.first_row, self._fit.n_rows, self._fit.capacity = self.hz, int(self._stitch.first_row), 0, int(trajectory)
            self._fit.flags |= capi.FIT_ACCUMULATE
            self.fit_traj = torch.zeros((B, int(trajectory), capi.FIT_COLS), **f64)
            self.fit_status = torch.zeros((B, int(trajectory)), dtype=torch.int32, device=dev)
            self.fit_summary = torch.from_numpy(force_fit.empty_summary(B).view(np.float64).reshape(B, 4, 3).copy()).to(dev)
            self._fit_scale = None if scale is None else torch.as_tensor(np.broadcast_to(np.asarray(scale, np.float64), (B,)).copy(), **f64)
        self.stream = stream if stream is not None else torch.cuda.current_stream(dev)
        self.have_plan = False
        self.x_range = x_range     # (lo, hi): a window that walks past an end of its heightfield turns round (no resets)
        self.warm_mode = warm      # "none": towr's straight-line guess (default); "shifted": the time-shifted previous plan
        self.solved = torch.zeros((), dtype=torch.int64, device=dev)
        self.iter_sum = torch.zeros((), dtype=torch.int64, device=dev)
        # the tensors above were filled on the caller's current stream; replan() works on self.stream (a non-blocking
        # torch.cuda.Stream is not ordered behind the default stream): finish that work here, once.  (A host wait, not
        # stream.wait_stream: a set's stream that has once waited on the default stream no longer ran side by side with the
        # other sets' streams on this runtime -- four sets took 28 ms per replan instead of 17.)
        torch.cuda.current_stream(dev).synchronize()

    def _init_path(self, path, path_base, path_hold, advance):
        """Upload the path table and the height grids (once) and fix the parameters of the path-goal calls."""
        torch, dev, B = self.torch, self.dev, self.B
        self.P._need("qtos_path_goal_device", "path-goal kernel")
        if path_base not in capi.PATH_BASES:
            raise ValueError("path_base is 'spine' or 'state'")
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        up = lambda a, kw: None if a is None else torch.as_tensor(np.ascontiguousarray(a), **kw).contiguous()
        plan = path.get("plan")
        self._path_plan_params = None
        if plan is not None:
            if path.get("table") is not None or path.get("path_id") is not None:
                raise ValueError("path['plan'] builds the table on the device, one path per window: give no path['table'] or path['path_id']")
            table = self._init_path_plan(path, plan)
        else:
            table = path["table"]
            self._path_knots, self._path_coef = up(table["knots"], f64), up(table["coef"], f64)
            self._path_n, self._path_rg = up(table["n_pieces"], i32), up(table.get("robot_goal"), f64)
        self.path_id = up(path.get("path_id"), i32)
        grids = path.get("map_yx")
        if grids is not None:
            grids = np.asarray(grids, np.float64)
            grids = grids[None] if grids.ndim == 2 else grids
        self._path_grids = up(grids, f64)
        self.path_map_id = up(path.get("map_id"), i32) if grids is not None else None
        for t, n in ((self.path_id, "path_id"), (self.path_map_id, "map_id")):
            if t is not None and tuple(t.shape) != (B,):
                raise ValueError("path['%s'] has one entry per window" % n)
        kw = dict(horizon=path.get("horizon", self.P.dims.duration), step_size=path["step_size"], tol=path.get("tol", 1e-5),
                  z_offset=path.get("z_offset", 0.24), cell=path.get("cell", 0.1), origin=path.get("origin", (1.0, 1.0)),
                  t_stop=5.0 + advance,     # (the reference stops once max_t < runtime - 5.0, and a plan starts `advance` ahead of the runtime)
                  stop_dist=path.get("stop_dist", 0.0), clamp_x=path.get("clamp_x", False), advance_clock=True,
                  hold_done=path_hold, table=table, map_yx=grids)
        self.path_params_init = capi.path_goal_params(base="state", **kw)      # plan_init: from the start state, at clock 0
        self.path_params = capi.path_goal_params(base=path_base, **kw)
        self.clock = torch.zeros((B,), **f64)
        self.done = torch.zeros((B,), **i32)
        if plan is not None:
            # (on the caller's current stream, as the uploads above: __init__ ends with a wait for it)
            self._path_plan(C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))

    def _init_path_plan(self, path, plan):
        """The buffers and parameters of the device path planner (k_path_plan): the table k_path_goal reads is written on the
        device, one path per window.  Returns what stands for the table where only its sizes are read."""
        torch, dev, B = self.torch, self.dev, self.B
        self.P._need("qtos_path_plan_device", "path-plan kernel")
        f64 = dict(dtype=torch.float64, device=dev)
        i32 = dict(dtype=torch.int32, device=dev)
        maps = np.asarray(plan["bool_map"], np.float64)
        maps = maps[None] if maps.ndim == 2 else maps
        rg = np.asarray(plan["robot_goal"], np.float64)
        if rg.shape != (B, 3):
            raise ValueError("path['plan']['robot_goal'] is B x 3")
        g = capi.path_plan_params(step_size=path["step_size"], cell=path.get("cell", 0.1), origin=path.get("origin", (1.0, 1.0)),
                                  height_bound=plan.get("height_bound", 0.2), max_cells=plan.get("max_cells"),
                                  max_open=plan.get("max_open", 4096), max_pieces=plan.get("max_pieces"), set_done=True, bool_map=maps)
        self._path_plan_params = g
        mp = int(g.max_pieces)
        self._plan_maps = torch.as_tensor(np.ascontiguousarray(maps), **f64).contiguous()
        mid = plan.get("map_id")
        self._plan_map_id = None if mid is None else torch.as_tensor(np.ascontiguousarray(mid), **i32).contiguous()
        if self._plan_map_id is not None and tuple(self._plan_map_id.shape) != (B,):
            raise ValueError("path['plan']['map_id'] has one entry per window")
        self._path_knots, self._path_coef = torch.zeros((B, mp + 1), **f64), torch.zeros((B, 2, 4, mp), **f64)
        self._path_n = torch.ones((B,), **i32)
        self._path_rg = torch.as_tensor(np.ascontiguousarray(rg), **f64).contiguous()
        self.path_cells = torch.zeros((B, int(g.max_cells), 2), **i32)
        self.path_n_cells, self.path_status = torch.zeros((B,), **i32), torch.zeros((B,), **i32)
        return dict(coef=np.broadcast_to(0.0, (B, 2, 4, mp)))

    def _path_plan(self, sp):
        """Queue k_path_plan: every window's path from self.start[:, 0:2] to its robot goal, into the table k_path_goal reads."""
        self.P._chk(self.P.lib.qtos_path_plan_device(self.P.h, self.B, C.byref(self._path_plan_params), ptr(self._plan_maps),
                                                     ptr(self._plan_map_id), ptr(self.start), ptr(self._path_rg), ptr(self._path_knots),
                                                     ptr(self._path_coef), ptr(self._path_n), ptr(self.path_cells), ptr(self.path_n_cells),
                                                     ptr(self.path_status), ptr(self.done), sp), "qtos_path_plan_device")

    def repath(self, robot_goal=None, bool_map=None):
        """Plan every window's path anew from where it stands, self.start[:, 0:2], on the set's stream (PATH_Solver.solve,
        QTOS/planner.py:422-457): to new robot goals (B x 3) and / or over new boolean maps (the shape given at creation; numpy,
        or a float64 tensor on the set's device, which is copied on the set's stream with no host copy), or the old ones.  A
        tensor is taken as the work queued on the caller's current stream leaves it (feasibility.feasibility_maps_device's
        result, say): where that is not the set's stream, the host waits for it once, and the caller may drop the tensor as soon
        as repath() returns.  The windows' clock starts again at 0 and their done bits are cleared (a window without a path gets
        bit 2 back).  Refused while a replan is pending."""
        torch = self.torch
        if self.path is None or self._path_plan_params is None:
            raise RuntimeError("repath() needs the device path planner (path=dict(plan=...))")
        if getattr(self, "_pending", False):
            raise RuntimeError("repath() while a replan is pending: poll() it first")
        made_on = torch.cuda.current_stream(self.dev)        # (where the caller's work stands: a bool_map tensor is made there)
        with torch.cuda.stream(self.stream):
            if robot_goal is not None:
                rg = np.ascontiguousarray(robot_goal, np.float64)
                if rg.shape != (self.B, 3):
                    raise ValueError("robot_goal is B x 3")
                self._path_rg.copy_(torch.from_numpy(rg))
            if torch.is_tensor(bool_map):
                # (a tensor on the set's device -- feasibility.feasibility_maps_device's --: copied on the set's stream)
                maps = bool_map[None] if bool_map.dim() == 2 else bool_map
                if maps.device != self._plan_maps.device or maps.dtype != self._plan_maps.dtype:
                    raise ValueError("a bool_map tensor is float64 on the set's device, %s" % (self._plan_maps.device,))
                if tuple(maps.shape) != tuple(self._plan_maps.shape):
                    raise ValueError("bool_map has the shape given at creation, %s" % (tuple(self._plan_maps.shape),))
                if made_on != self.stream:
                    # the tensor is written by work on the caller's stream and read by the copy on the set's.  A host wait, not
                    # stream.wait_stream, for the reason __init__ gives: a set's stream that has once waited on the default stream
                    # no longer ran side by side with the other sets' streams.  record_stream: the allocator keeps the tensor's
                    # block out of the caller's pool until the copy has run, whatever the caller does with the tensor meanwhile
                    made_on.synchronize()
                    maps.record_stream(self.stream)
                self._plan_maps.copy_(maps)
            elif bool_map is not None:
                maps = np.ascontiguousarray(bool_map, np.float64)
                maps = maps[None] if maps.ndim == 2 else maps
                if maps.shape != tuple(self._plan_maps.shape):
                    raise ValueError("bool_map has the shape given at creation, %s" % (tuple(self._plan_maps.shape),))
                self._plan_maps.copy_(torch.from_numpy(maps))
            self.clock.zero_()
            self.done.zero_()
            self._path_plan(C.c_void_p(self.stream.cuda_stream))

    def _path_goal(self, params, offset, sp):
        """Queue k_path_goal: the goals of the plans about to be asked for, from self.start (and the hand-over's offset)."""
        self.P._chk(self.P.lib.qtos_path_goal_device(self.P.h, self.B, C.byref(params), ptr(self._path_knots), ptr(self._path_coef),
                                                     ptr(self._path_n), ptr(self._path_rg), ptr(self.path_id), ptr(self._path_grids),
                                                     ptr(self.path_map_id), ptr(self.clock), ptr(offset), ptr(self.start), ptr(self.goal),
                                                     ptr(self.done), sp), "qtos_path_goal_device")

    def _joint_rows(self, params, n_rows, sp):
        """Queue k_joint_rows in front of a stitch: the joint rows of the segment that stitch appends, to the same ring rows (the
        kernel reads the cursor and the clock the stitch behind it moves on)."""
        self.P._chk(self.P.lib.qtos_joint_rows_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(), None,
                                                      n_rows, self.cursor.data_ptr(), None, None, self.joint_traj.data_ptr(),
                                                      self.joint_status.data_ptr(), sp), "qtos_joint_rows_device")

    def joint_rows(self, b):
        """Window b's newest min(cursor, trajectory) joint rows in time order and their status words, as numpy (the stream is
        synchronised): row for row the joint commands of ``trajectory_rows(b)``."""
        from .stitcher import ring_rows
        if self.joint_traj is None:
            raise RuntimeError("joint_rows() needs the joint ring (joints=...)")
        self.stream.synchronize()
        cur = int(self.cursor[b].item())
        return ring_rows(self.joint_traj[b].cpu().numpy(), cur), ring_rows(self.joint_status[b].cpu().numpy(), cur)

    def _track_rows(self, params, n_rows, sp):
        """Queue k_track in front of a stitch (behind the joint rows): the track rows of the segment that stitch appends, from the
        measured ring's rows of that segment, to the same ring rows."""
        if self._track_fill is not None:
            self._track_fill(self)
        self.P._chk(self.P.lib.qtos_track_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(), None, n_rows,
                                                 self.cursor.data_ptr(), self.meas_traj.data_ptr(),
                                                 ptr(self.track_goal_x),
                                                 self.track_count.data_ptr(), self.track_total.data_ptr(), self.track_traj.data_ptr(),
                                                 self.track_status.data_ptr(), sp), "qtos_track_device")

    def _rollout_rows(self, params, n_rows, sp):
        """Queue k_rollout in front of a stitch, behind the joint rows and in front of the track call: the bodies go on from the
        state they carry over the rows that stitch appends, under the plan handed over from, and their states fill the measured
        ring's rows of the segment (the joint columns from the joint ring where ``joints`` is on).  A window's first call with
        rows sets its state from the plan's row: ``rollout_word`` starts as QTOS_ROLLOUT_PENDING, which the kernel spends per
        window, so a window whose hand-over row is 0 at the set's first replan is set on its plan by a later one.  With ``feet``
        k_rollout_feet is queued in its place, with the same carried arrays, and fills ``rollout_feet_traj`` as well; with
        ``limit="qp"`` k_rollout_qp, which fills ``rollout_qp_traj`` too."""
        if self._feet is not None and self._feet_qp:
            f = self._feet.with_body(params)
            self.P._chk(self.P.lib.qtos_rollout_qp_device(self.P.h, self.B, C.byref(f), self.nodes.data_ptr(), self.t0.data_ptr(), None, n_rows,
                                                          self.cursor.data_ptr(), ptr(self.joint_traj), ptr(self._rollout_scale),
                                                          ptr(self._rollout_push), self.rollout_state.data_ptr(),
                                                          self.rollout_count.data_ptr(), self.rollout_word.data_ptr(),
                                                          self.meas_traj.data_ptr(), ptr(self.rollout_traj),
                                                          self.rollout_feet_traj.data_ptr(), self.rollout_qp_traj.data_ptr(),
                                                          self.rollout_status.data_ptr(), sp), "qtos_rollout_qp_device")
            return
        if self._feet is not None:
            f = self._feet.with_body(params)
            self.P._chk(self.P.lib.qtos_rollout_feet_device(self.P.h, self.B, C.byref(f), self.nodes.data_ptr(), self.t0.data_ptr(), None, n_rows,
                                                            self.cursor.data_ptr(), ptr(self.joint_traj), ptr(self._rollout_scale),
                                                            ptr(self._rollout_push), self.rollout_state.data_ptr(),
                                                            self.rollout_count.data_ptr(), self.rollout_word.data_ptr(),
                                                            self.meas_traj.data_ptr(), ptr(self.rollout_traj),
                                                            self.rollout_feet_traj.data_ptr(), self.rollout_status.data_ptr(), sp),
                        "qtos_rollout_feet_device")
            return
        self.P._chk(self.P.lib.qtos_rollout_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(), None, n_rows,
                                                   self.cursor.data_ptr(), ptr(self.joint_traj), ptr(self._rollout_scale),
                                                   ptr(self._rollout_push), self.rollout_state.data_ptr(), self.rollout_count.data_ptr(),
                                                   self.rollout_word.data_ptr(), self.meas_traj.data_ptr(), ptr(self.rollout_traj),
                                                   self.rollout_status.data_ptr(), sp), "qtos_rollout_device")

    def rollout_rows(self, b):
        """Window b's newest min(cursor, trajectory) rollout rows in time order (None without ``rows=True``) and their status
        words, as numpy (the stream is synchronised): row for row the simulated states of ``trajectory_rows(b)``."""
        from .stitcher import ring_rows
        if self._rollout is None:
            raise RuntimeError("rollout_rows() needs the rollout (rollout=dict(...))")
        self.stream.synchronize()
        cur = int(self.cursor[b].item())
        rows = None if self.rollout_traj is None else ring_rows(self.rollout_traj[b].cpu().numpy(), cur)
        return rows, ring_rows(self.rollout_status[b].cpu().numpy(), cur)

    def rollout_feet_rows(self, b):
        """Window b's newest min(cursor, trajectory) feet rows (16 columns: time stamp, applied forces, what the feet did not
        deliver) in time order, as numpy (the stream is synchronised): row for row with ``rollout_rows(b)``."""
        from .stitcher import ring_rows
        if self._rollout is None or self._feet is None:
            raise RuntimeError("rollout_feet_rows() needs the rollout through the feet (rollout=dict(..., feet=dict(...)))")
        self.stream.synchronize()
        return ring_rows(self.rollout_feet_traj[b].cpu().numpy(), int(self.cursor[b].item()))

    def rollout_qp_rows(self, b):
        """Window b's newest min(cursor, trajectory) solve rows (8 columns, force_qp.py's QP_COLS, of every tick's first step) in
        time order, as numpy (the stream is synchronised): row for row with ``rollout_feet_rows(b)``."""
        from .stitcher import ring_rows
        if self._rollout is None or self._feet is None or not self._feet_qp:
            raise RuntimeError("rollout_qp_rows() needs the rollout with the force QP (rollout=dict(..., feet=dict(limit=\"qp\", ...)))")
        self.stream.synchronize()
        return ring_rows(self.rollout_qp_traj[b].cpu().numpy(), int(self.cursor[b].item()))

    def _start_feedback(self, sp):
        """Queue k_start_feedback behind the track call and in front of the stitch: self.start (and, without a path, self.goal)
        from the measured ring's row of the hand-over (the kernel reads the cursor and the clock the stitch behind it moves on)."""
        moves = self.path is None
        self.P._chk(self.P.lib.qtos_start_feedback_device(self.P.h, self.B, C.byref(self._feedback), self.nodes.data_ptr(), self.t0.data_ptr(),
                                                          self.row.data_ptr(), self.cursor.data_ptr(), self.meas_traj.data_ptr(),
                                                          ptr(self.map_id), self.start.data_ptr(),
                                                          self.goal_step.data_ptr() if moves else None,
                                                          self.goal.data_ptr() if moves else None, self.feedback_err.data_ptr(),
                                                          self.feedback_status.data_ptr(), sp), "qtos_start_feedback_device")

    def _plan_check(self, params, n_rows, sp):
        """Queue k_plan_check in front of a stitch: the rows that stitch appends, merged into the windows' records (the kernel
        reads the cursor and the clock the stitch behind it moves on; no table is written)."""
        self.P._chk(self.P.lib.qtos_plan_check_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(),
                                                      ptr(self.map_id), None, n_rows,
                                                      self.cursor.data_ptr(), None, self.check_summary.data_ptr(), sp),
                    "qtos_plan_check_device")

    def _force_fit(self, params, n_rows, sp):
        """Queue k_force_fit in front of a stitch, behind the joint rows: the fit rows of the segment that stitch appends, to the
        same ring rows, with the joint ring's angles where ``joints`` is on, merged into the windows' records (the kernel reads the
        cursor and the clock the stitch behind it moves on)."""
        if isinstance(params, capi.QtosForceQp):
            self.P._chk(self.P.lib.qtos_force_qp_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(),
                                                        ptr(self.map_id), None, n_rows, self.cursor.data_ptr(), ptr(self.joint_traj),
                                                        ptr(self._fit_scale), self.fit_traj.data_ptr(), self.qp_traj.data_ptr(),
                                                        self.fit_status.data_ptr(), self.fit_summary.data_ptr(), sp), "qtos_force_qp_device")
            return
        self.P._chk(self.P.lib.qtos_force_fit_device(self.P.h, self.B, C.byref(params), self.nodes.data_ptr(), self.t0.data_ptr(),
                                                     ptr(self.map_id), None, n_rows, self.cursor.data_ptr(), ptr(self.joint_traj),
                                                     ptr(self._fit_scale), self.fit_traj.data_ptr(), self.fit_status.data_ptr(),
                                                     self.fit_summary.data_ptr(), sp), "qtos_force_fit_device")

    def fit_rows(self, b):
        """Window b's newest min(cursor, trajectory) fit rows in time order and their status words, as numpy (the stream is
        synchronised): row for row the fitted forces of ``trajectory_rows(b)``."""
        from .stitcher import ring_rows
        if self._fit is None:
            raise RuntimeError("fit_rows() needs the force fit (fit=...)")
        self.stream.synchronize()
        cur = int(self.cursor[b].item())
        return ring_rows(self.fit_traj[b].cpu().numpy(), cur), ring_rows(self.fit_status[b].cpu().numpy(), cur)

    def qp_rows(self, b):
        """Window b's newest min(cursor, trajectory) rows of the force QP's solve table (8 columns, force_qp.py) in time order, as
        numpy (the stream is synchronised): row for row with ``fit_rows(b)``."""
        from .stitcher import ring_rows
        if not isinstance(self._fit, capi.QtosForceQp):
            raise RuntimeError("qp_rows() needs the force fit with limits (fit=dict(limits=...))")
        self.stream.synchronize()
        return ring_rows(self.qp_traj[b].cpu().numpy(), int(self.cursor[b].item()))

    def fit_worst(self):
        """What the fit left and changed over the windows' executed rows so far, [B, 4] records of force_fit.SUMMARY (the families
        res_ang, res_lin, change, excess: the largest value, the trajectory row -- the window's clock, as ``cursor`` counts it --
        that attains it, the rows over the tolerance), as numpy (the stream is synchronised)."""
        from . import force_fit
        if self._fit is None:
            raise RuntimeError("fit_worst() needs the force fit (fit=...)")
        self.stream.synchronize()
        return self.fit_summary.cpu().numpy().view(force_fit.SUMMARY).reshape(self.B, 4)

    def check_worst(self):
        """What the windows' executed rows violated so far, [B, 5] records of plan_check.SUMMARY (the families dyn_ang, dyn_lin,
        rom, terrain, force: the largest violation, the trajectory row -- the window's clock, as ``cursor`` counts it -- that
        attains it, the rows over the tolerance), as numpy (the stream is synchronised)."""
        from . import plan_check
        if self._check is None:
            raise RuntimeError("check_worst() needs the plan check (check=capi.check_params(...))")
        self.stream.synchronize()
        return self.check_summary.cpu().numpy().view(plan_check.SUMMARY).reshape(self.B, 5)

    def track_rows(self, b):
        """Window b's newest min(cursor, trajectory) track rows in time order and their status words, as numpy (the stream is
        synchronised): row for row the measured poses and errors of ``trajectory_rows(b)``."""
        from .stitcher import ring_rows
        if self.track_traj is None:
            raise RuntimeError("track_rows() needs the track ring (track=...)")
        self.stream.synchronize()
        cur = int(self.cursor[b].item())
        return ring_rows(self.track_traj[b].cpu().numpy(), cur), ring_rows(self.track_status[b].cpu().numpy(), cur)

    def replan(self):
        """One replan of every window: begin() + poll() until the call is queued to its end (results: synchronise the stream)."""
        self.begin()
        self.P.wait()          # (inside the library: the GIL is released, other sets' host threads are not held up)
        self.poll()
        return self.nodes, self.status

    def begin(self):
        """Queue the next replan (hand-over rows, new start / goal vectors, the whole solve) on the set's stream and return
        at once: several sets of windows are kept in flight by ONE host thread that begins / polls them in turn."""
        with self.torch.cuda.stream(self.stream):     # (several window sets may run side by side, each on its own stream)
            self._begin()
        self._pending = True

    def poll(self):
        """True once the replan begun last has been queued to its end (qtos_plan_poll); tallies its results on the stream."""
        if not getattr(self, "_pending", False):
            return True
        if not self.P.poll():
            return False
        with self.torch.cuda.stream(self.stream):
            self.solved.add_((self.status == 0).sum())
            self.iter_sum.add_(self.iters.sum())
        self.have_plan = True
        self._pending = False
        return True

    def finish(self):
        """The end of the loop (with ``trajectory``): append the rest of the newest plan, its rows first_row .. the last, to
        every window's ring.  The clock stays: ``t0`` is still the time stamp of that plan's row 0."""
        if self.traj is None:
            raise RuntimeError("finish() needs a trajectory ring (trajectory=...)")
        if getattr(self, "_pending", False) or not self.have_plan:
            raise RuntimeError("finish() needs a finished replan: poll() it first")
        n_all = int(round(self.P.dims.duration * self.hz)) + 1
        first, cap = int(self._stitch.first_row), int(self._stitch.capacity)
        while first < n_all:        # (a call appends at most `capacity` rows: a plan longer than the ring goes in pieces, its newest rows stay)
            n = min(n_all - first, cap)
            s = capi.stitch_params(cap, first, n, self.hz, False)
            if self.joint_traj is not None:
                g = self._joint.copy()
                g.first_row, g.n_rows = first, n
                self._joint_rows(g, None, C.c_void_p(self.stream.cuda_stream))
            if self._rollout is not None:
                g = self._rollout.copy()
                g.first_row, g.n_rows = first, n
                self._rollout_rows(g, None, C.c_void_p(self.stream.cuda_stream))
            if self.track_traj is not None:
                g = self._track.copy()
                g.first_row, g.n_rows = first, n
                with self.torch.cuda.stream(self.stream):
                    self._track_rows(g, None, C.c_void_p(self.stream.cuda_stream))
            if self._fit is not None:
                g = self._fit.copy()
                g.first_row, g.n_rows = first, n
                self._force_fit(g, None, C.c_void_p(self.stream.cuda_stream))
            if self._check is not None:
                g = self._check.copy()
                g.first_row, g.n_rows = first, n
                self._plan_check(g, None, C.c_void_p(self.stream.cuda_stream))
            self.P._chk(self.P.lib.qtos_stitch_device(self.P.h, self.B, C.byref(s), self.nodes.data_ptr(), None, self.t0.data_ptr(),
                                                      self.traj.data_ptr(), self.cursor.data_ptr(), C.c_void_p(self.stream.cuda_stream)),
                        "qtos_stitch_device")
            first += n

    def trajectory_rows(self, b):
        """Window b's newest min(cursor, trajectory) rows in time order, as numpy (the stream is synchronised)."""
        from .stitcher import ring_rows
        if self.traj is None:
            raise RuntimeError("trajectory_rows() needs a trajectory ring (trajectory=...)")
        self.stream.synchronize()
        return ring_rows(self.traj[b].cpu().numpy(), int(self.cursor[b].item()))

    def _handover_rows(self, sp):
        """The hand-over through the sampled row table (handover="rows"): what _begin did before k_handover."""
        torch, P, B = self.torch, self.P, self.B
        # hand-over rows: sample the newest plan from `advance` on, take the first row with all feet in contact
        # (force columns 25.. of a foot are non-zero exactly in stance: the reference tests foot heights against
        # the terrain's height set, QTOS/combiner.py:78-92 -- the same rows on these maps)
        n_rows = self.rows.shape[1]
        self.P._chk(P.lib.qtos_sample_csv_device(P.h, B, self.nodes.data_ptr(), self.t0.data_ptr(), C.c_double(self.hz), n_rows,
                                                 self.rows.data_ptr(), sp), "qtos_sample_csv_device")
        k0 = n_rows - self.n_search - 1
        cand = self.rows[:, k0:, :]
        contact = (cand[:, :, 25:37].reshape(B, -1, 4, 3)[..., 2] > 0).all(dim=2)
        first = torch.where(contact.any(dim=1), contact.to(torch.int32).argmax(dim=1), torch.zeros((B,), dtype=torch.int64, device=self.dev))
        idx = k0 + first
        hand = self.rows[torch.arange(B, device=self.dev), idx]
        self.start.copy_(hand[:, 1:25])
        self.offset.copy_(idx.to(torch.float64) / self.hz)
        if self.traj is not None:
            self.row.copy_(idx)
        if self.path is not None:
            return                       # (the goals come from k_path_goal)
        if self.x_range is not None:
            lo, hi = self.x_range
            x = self.start[:, 0]
            sgn = torch.where(x > hi, -torch.ones_like(x), torch.where(x < lo, torch.ones_like(x), torch.sign(self.goal_step[:, 0])))
            self.goal_step[:, 0] = sgn * self.goal_step[:, 0].abs()
        self.goal[:, 0:2] = self.start[:, 0:2] + self.goal_step[:, 0:2]

    def _begin(self):
        torch, P, B = self.torch, self.P, self.B
        sp = C.c_void_p(self.stream.cuda_stream)
        warm_ptr = None
        if self.have_plan:
            if self.handover == "kernel":
                # hand-over: k_handover picks every window's row of its newest plan, evaluates it into start and moves the goal
                # (with a path: without goal_step, the goal is k_path_goal's)
                self.P._chk(P.lib.qtos_handover_device(P.h, B, C.byref(self._hand), self.nodes.data_ptr(),
                                                       None if self.path is not None else self.goal_step.data_ptr(),
                                                       self.start.data_ptr(), None if self.path is not None else self.goal.data_ptr(),
                                                       self.offset.data_ptr(), self.row.data_ptr(), sp), "qtos_handover_device")
            else:
                self._handover_rows(sp)
            if self.path is not None and self._feedback is None:
                # where the next plan goes: the window's path one horizon ahead of the hand-over, behind it on the same stream
                self._path_goal(self.path_params, self.offset, sp)
            if self.traj is not None:
                # the rows executed of the plan handed over from go to the windows' rings; t0 moves on to the new plan's row 0
                if self.joint_traj is not None:
                    self._joint_rows(self._joint, self.row.data_ptr(), sp)
                if self._rollout is not None:
                    self._rollout_rows(self._rollout, self.row.data_ptr(), sp)
                if self.track_traj is not None:
                    self._track_rows(self._track, self.row.data_ptr(), sp)
                if self._feedback is not None:
                    # the start moves to where the robot is; the path goal follows it, so that path_base="state" sees it
                    self._start_feedback(sp)
                    if self.path is not None:
                        self._path_goal(self.path_params, self.offset, sp)
                if self._fit is not None:
                    self._force_fit(self._fit, self.row.data_ptr(), sp)
                if self._check is not None:
                    self._plan_check(self._check, self.row.data_ptr(), sp)
                self.P._chk(P.lib.qtos_stitch_device(P.h, B, C.byref(self._stitch), self.nodes.data_ptr(), self.row.data_ptr(),
                                                     self.t0.data_ptr(), self.traj.data_ptr(), self.cursor.data_ptr(), sp),
                            "qtos_stitch_device")
            self.nodes, self.prev = self.prev, self.nodes
            if self.warm_mode == "shifted":
                self.P._chk(P.lib.qtos_shift_warm_device(P.h, B, self.prev.data_ptr(), self.offset.data_ptr(), self.start.data_ptr(),
                                                         self.goal.data_ptr(), ptr(self.map_id),
                                                         self.warm.data_ptr(), sp), "qtos_shift_warm_device")
                mix = getattr(self, "_mix", "all")
                if mix != "all":     # (scratch/shift_exp.py: only part of the shifted plan, the rest from the straight-line guess)
                    guess = torch.empty_like(self.warm)
                    big = torch.full_like(self.offset, 1e9)
                    self.P._chk(P.lib.qtos_shift_warm_device(P.h, B, self.prev.data_ptr(), big.data_ptr(), self.start.data_ptr(),
                                                             self.goal.data_ptr(), ptr(self.map_id),
                                                             guess.data_ptr(), sp), "qtos_shift_warm_device")
                    nbn = P.dims.n_base_nodes
                    if mix == "cold":
                        self.warm.copy_(guess)
                    elif mix == "base":
                        self.warm[:, 12 * nbn:] = guess[:, 12 * nbn:]
                    elif mix == "base+feet":
                        self.warm[:, self._force_off:] = guess[:, self._force_off:]
                warm_ptr = self.warm.data_ptr()
        elif self.path is not None:
            self._path_goal(self.path_params_init, None, sp)
        self.P._chk(P.lib.qtos_plan_submit(P.h, B, self.start.data_ptr(), self.goal.data_ptr(),
                                           ptr(self.map_id), warm_ptr,
                                           self.nodes.data_ptr(), self.status.data_ptr(), self.iters.data_ptr(),
                                           self.viol.data_ptr(), sp), "qtos_plan_submit")
