"""The mirror of include/qtos_planner.h in ctypes, stated once: its constants, its structures and the prototype of every
entry point.  Nothing else lives here; capi.py re-exports all of it and builds on it.  tests/test_abi_cpu.py holds the three
to the header: every #define, every field's offset and size, every declaration's arguments and return value."""
import ctypes as C

# every #define QTOS_* of the header by its name there; the module's own names drop the prefix (NEE, TRACK_COLS, ...)
CONSTANTS = {
    "QTOS_NEE": 4, "QTOS_MAX_PHASES": 32, "QTOS_START_DOUBLES": 24, "QTOS_CSV_COLS": 37,
    "QTOS_HIST_COLS": 10,                 # one record of the iteration history (qtos_plan_report)
    "QTOS_JOINT_NO_FF": 1,
    "QTOS_JOINT_NONFINITE": 4096,         # leg 0's bit in the status word of a joint row; leg e: << e
    "QTOS_TRACK_QUAT": 1, "QTOS_TRACK_CLEAN_DELAY": 2, "QTOS_TRACK_COLS": 26,
    "QTOS_FEEDBACK_QUAT": 1, "QTOS_FEEDBACK_SNAP": 2, "QTOS_FEEDBACK_ZERO_FILTER": 4,
    "QTOS_CHECK_ACCUMULATE": 1, "QTOS_CHECK_COLS": 27, "QTOS_CHECK_FAMILIES": 5,
    "QTOS_ROLLOUT_INIT": 1, "QTOS_ROLLOUT_QUAT": 2,
    "QTOS_ROLLOUT_PENDING": 32,           # in a window's carried word, spent by its first call with rows
    "QTOS_ROLLOUT_COLS": 20, "QTOS_ROLLOUT_STATE": 13,
    "QTOS_FEET_LIMIT": 1, "QTOS_ROLLOUT_FEET_COLS": 16,
    "QTOS_ROLLOUT_NO_STANCE": 64, "QTOS_ROLLOUT_TWO_STANCE": 128, "QTOS_ROLLOUT_LIMITED": 256,      # status bits of a feet rollout's row
    "QTOS_FIT_ACCUMULATE": 1, "QTOS_FIT_COLS": 32, "QTOS_FIT_FAMILIES": 4,
    "QTOS_QP_COLS": 8, "QTOS_QP_MAX_ITER": 25,
    "QTOS_QP_NO_STANCE": 1, "QTOS_QP_TWO_STANCE": 2, "QTOS_QP_NONFINITE": 4, "QTOS_QP_ACTIVE": 8, "QTOS_QP_CAP": 128,
    "QTOS_QP_LIMITED": 256,               # status bits of a force-QP row
    "QTOS_ROLLOUT_QP_COLS": 8, "QTOS_ROLLOUT_CAP": 512,       # a rollout with the force QP: its solve table, its status bit
    "QTOS_ENV_MAX_LEVELS": 64, "QTOS_ENV_MAX_DRAWS": 1 << 24, "QTOS_ENV_LDS_BYTES": 3568,
}
globals().update({name[len("QTOS_"):]: value for name, value in CONSTANTS.items()})
NEE, MAX_PHASES = CONSTANTS["QTOS_NEE"], CONSTANTS["QTOS_MAX_PHASES"]      # (the two the structures below are sized by)


class _Struct(C.Structure):
    def copy(self):
        return type(self).from_buffer_copy(self)


class QtosParams(_Struct):
    _fields_ = [
        ("n_phases", C.c_int * NEE),
        ("phase_dur", (C.c_double * MAX_PHASES) * NEE),
        ("dt_base", C.c_double), ("dt_dyn", C.c_double), ("dt_rom", C.c_double),
        ("force_polys_per_stance", C.c_int),
        ("mass", C.c_double), ("gravity", C.c_double), ("inertia_b", C.c_double * 9),
        ("nominal_stance", (C.c_double * 3) * NEE), ("max_dev", C.c_double * 3),
        ("mu", C.c_double), ("f_max", C.c_double), ("t_swing_avg", C.c_double),
        ("honor_start_velocity", C.c_int), ("terrain_mode", C.c_int),
        ("max_iter", C.c_int),
        ("tol", C.c_double), ("mu_init", C.c_double), ("mu_min", C.c_double),
        ("delta_x", C.c_double), ("eps_dual", C.c_double), ("slack_push", C.c_double), ("warm_slack_push", C.c_double),
        ("stall_iters", C.c_int), ("hold_from", C.c_int), ("hold_weight", C.c_double), ("hold_tol", C.c_double),
        ("chord_tol", C.c_double),
        ("reduce_base", C.c_int),
        ("chord_max", C.c_int), ("chord_shrink", C.c_double), ("stall_alpha", C.c_double),
        ("reduce_swing", C.c_int),
        ("mu_superlinear", C.c_int),
        ("kappa_sigma", C.c_double),
    ]


class QtosDims(_Struct):
    _fields_ = [
        ("n_vars", C.c_int), ("n_cons", C.c_int),
        ("n_free", C.c_int), ("n_eq", C.c_int), ("n_ineq", C.c_int),
        ("n_ineq_lower", C.c_int), ("n_ineq_both", C.c_int), ("n_ineq_upper", C.c_int),
        ("n_eq_work", C.c_int), ("n_unknowns", C.c_int),
        ("n_stages", C.c_int), ("pivots", C.c_int), ("front", C.c_int),
        ("n_base_nodes", C.c_int), ("n_dyn_times", C.c_int), ("n_rom_times", C.c_int),
        ("n_rows_csv", C.c_int),
        ("panel_doubles", C.c_longlong), ("g_doubles", C.c_longlong),
        ("kkt_algorithmic_bytes", C.c_longlong), ("kkt_flops", C.c_longlong),
        ("envelope", C.c_longlong), ("max_active", C.c_int), ("order_rule", C.c_int),
        ("duration", C.c_double),
    ]


class QtosReport(_Struct):
    _fields_ = [
        ("status", C.c_int), ("iterations", C.c_int), ("n_rows", C.c_int),
        ("n_con_evals", C.c_int), ("n_jac_evals", C.c_int), ("n_factorizations", C.c_int), ("n_chord_solves", C.c_int),
        ("pad", C.c_int),
        ("constraint_violation", C.c_double), ("dual_infeasibility", C.c_double), ("complementarity", C.c_double),
        ("nlp_error", C.c_double),
    ]


class QtosSelftest(_Struct):
    """One attempt of the create-time KKT self-test (qtos_planner_selftest)."""
    _fields_ = [
        ("order_rule", C.c_int), ("front", C.c_int), ("n_stages", C.c_int), ("n_problems", C.c_int),
        ("worst_stage", C.c_int), ("passed", C.c_int),
        ("residual", C.c_double), ("residual_refined", C.c_double), ("max_factor", C.c_double),
        ("growth_limit", C.c_double), ("tol_residual", C.c_double), ("seconds", C.c_double),
    ]

    def describe(self):
        if not self.front:
            return "rule %d, not built" % self.order_rule
        return "rule %d, residual %.1e, max |V| %.2e, %s" % (self.order_rule, self.residual, self.max_factor,
                                                              "passed" if self.passed else "rejected (stage %d)" % self.worst_stage)


class QtosHandover(_Struct):
    """Parameters of a replan's hand-over (qtos_handover*)."""
    _fields_ = [
        ("advance", C.c_double), ("search", C.c_double), ("hz", C.c_double),
        ("rule", C.c_int), ("n_heights", C.c_int), ("heights", C.c_double * 8),
        ("zero_filter", C.c_int), ("turn", C.c_int), ("x_lo", C.c_double), ("x_hi", C.c_double),
    ]


class QtosStitch(_Struct):
    """Parameters of a stitch call (qtos_stitch*)."""
    _fields_ = [
        ("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("advance_clock", C.c_int), ("capacity", C.c_longlong),
    ]


class QtosPathGoal(_Struct):
    """Parameters of a path-goal call (qtos_path_goal*)."""
    _fields_ = [
        ("horizon", C.c_double), ("step_size", C.c_double), ("tol", C.c_double), ("z_offset", C.c_double),
        ("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double), ("t_stop", C.c_double), ("stop_dist", C.c_double),
        ("base", C.c_int), ("clamp_x", C.c_int), ("advance_clock", C.c_int), ("hold_done", C.c_int),
        ("n_paths", C.c_int), ("max_pieces", C.c_int), ("n_maps", C.c_int), ("rows", C.c_int), ("cols", C.c_int),
    ]


class QtosPathPlan(_Struct):
    """Parameters of a path-plan call (qtos_path_plan*)."""
    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("cell", C.c_double), ("origin_x", C.c_double), ("origin_y", C.c_double),
        ("height_bound", C.c_double), ("step_size", C.c_double), ("max_cells", C.c_int), ("max_open", C.c_int), ("max_pieces", C.c_int),
        ("n_maps", C.c_int), ("set_done", C.c_int),
    ]


class QtosProbe(_Struct):
    """Parameters of a probe / stamp call (qtos_probe*, qtos_probe_stamp*)."""
    _fields_ = [
        ("rows", C.c_int), ("cols", C.c_int), ("n_maps", C.c_int), ("cell", C.c_double), ("scale", C.c_int), ("multi_map_shift", C.c_int),
        ("origin_shift", C.c_double), ("z_offset", C.c_double), ("nominal_stance", (C.c_double * 3) * NEE),
    ]


class QtosTerrainEnv(_Struct):
    """Parameters of a terrain-env call (qtos_terrain_env*)."""
    _fields_ = [
        ("n_maps", C.c_int), ("n_base", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("n_shift", C.c_int), ("n_height", C.c_int),
        ("climb", C.c_int), ("delta", C.c_double),
    ]


class QtosJointRows(_Struct):
    """Parameters of a joint-rows call (qtos_joint_rows*); joints.joint_rows reads the same fields."""
    _fields_ = [
        ("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("capacity", C.c_longlong), ("ee_shift", C.c_double),
        ("hip", (C.c_double * 3) * 4), ("lateral", C.c_double * 4), ("l_upper", C.c_double), ("l_lower", C.c_double),
        ("knee_sign", C.c_double * 4), ("kp", C.c_double * 12), ("kd", C.c_double * 12), ("tau_max", C.c_double), ("flags", C.c_int),
    ]


class QtosTrack(_Struct):
    """Parameters of a track call (qtos_track*); tracking.track_rows reads the same fields."""
    _fields_ = [
        ("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("capacity", C.c_longlong), ("ee_shift", C.c_double),
        ("hip", (C.c_double * 3) * 4), ("lateral", C.c_double * 4), ("l_upper", C.c_double), ("l_lower", C.c_double),
        ("delay", C.c_int), ("flags", C.c_int),
    ]


class QtosFeedback(_Struct):
    """Parameters of a feedback hand-over (qtos_start_feedback*); feedback.start_feedback reads the same fields."""
    _fields_ = [
        ("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("capacity", C.c_longlong), ("latency", C.c_double),
        ("ee_shift", C.c_double), ("hip", (C.c_double * 3) * 4), ("lateral", C.c_double * 4), ("l_upper", C.c_double),
        ("l_lower", C.c_double), ("gain_pos", C.c_double), ("gain_ang", C.c_double), ("gain_foot", C.c_double),
        ("max_pos", C.c_double), ("max_ang", C.c_double), ("max_foot", C.c_double), ("nominal", (C.c_double * 3) * 4),
        ("max_deviation", C.c_double * 3), ("rom_tol", C.c_double), ("snap_tol", C.c_double), ("flags", C.c_int),
    ]


class QtosCheckRecord(_Struct):
    """One family of one window in a plan check's or a force fit's summary; plan_check.SUMMARY is its numpy dtype."""
    _fields_ = [("max", C.c_double), ("row", C.c_longlong), ("count", C.c_longlong)]


class QtosPlanCheck(_Struct):
    """Parameters of a plan check (qtos_plan_check*)."""
    _fields_ = [("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("tol", C.c_double * 5), ("flags", C.c_int)]


class QtosRollout(_Struct):
    """Parameters of a rollout (qtos_rollout*); rollout.rollout_rows reads the same fields."""
    _fields_ = [
        ("hz", C.c_double), ("substeps", C.c_int), ("first_row", C.c_int), ("n_rows", C.c_int), ("capacity", C.c_longlong),
        ("flags", C.c_int), ("mass", C.c_double), ("gravity", C.c_double), ("inertia_b", C.c_double * 9),
        ("inertia_b_inv", C.c_double * 9), ("ff_scale", C.c_double), ("kp_lin", C.c_double * 3), ("kd_lin", C.c_double * 3),
        ("kp_ang", C.c_double * 3), ("kd_ang", C.c_double * 3), ("f_fb_max", C.c_double), ("t_fb_max", C.c_double),
        ("dev_max", C.c_double), ("tilt_max", C.c_double), ("push_from", C.c_longlong), ("push_ticks", C.c_longlong),
    ]


class QtosRolloutFeet(_Struct):
    """Parameters of a rollout through the feet (qtos_rollout_feet*): QtosRollout's fields, then the feet's.
    rollout_feet.rollout_feet_rows takes it as its RolloutParams and as its FeetParams."""
    _fields_ = QtosRollout._fields_ + [
        ("arm", C.c_double), ("damping", C.c_double), ("w_min", C.c_double), ("mu", C.c_double), ("f_max", C.c_double),
        ("feet_flags", C.c_int),
    ]

    def with_body(self, body):
        """A copy whose QtosRollout part is `body` (a QtosRollout)."""
        g = self.copy()
        C.memmove(C.byref(g), C.byref(body), C.sizeof(QtosRollout))
        return g


class QtosRolloutQp(_Struct):
    """Parameters of a rollout with the force QP (qtos_rollout_qp*): QtosRolloutFeet's fields, then the QP's.
    rollout_qp.rollout_qp_rows takes it as its RolloutParams and as its QpFeetParams."""
    _fields_ = QtosRolloutFeet._fields_ + [("mu_end", C.c_double), ("act_tol", C.c_double), ("max_iter", C.c_int)]
    with_body = QtosRolloutFeet.with_body


class QtosForceFit(_Struct):
    """Parameters of a force fit (qtos_force_fit*); force_fit.fit_rows reads the same fields."""
    _fields_ = [
        ("hz", C.c_double), ("first_row", C.c_int), ("n_rows", C.c_int), ("capacity", C.c_longlong), ("flags", C.c_int),
        ("arm", C.c_double), ("damping", C.c_double), ("w_min", C.c_double), ("excess_tol", C.c_double), ("tol", C.c_double * 4),
        ("hip", (C.c_double * 3) * 4), ("lateral", C.c_double * 4), ("l_upper", C.c_double), ("l_lower", C.c_double),
        ("knee_sign", C.c_double * 4), ("ee_shift", C.c_double),
    ]


class QtosForceQp(_Struct):
    """Parameters of a force QP (qtos_force_qp*): QtosForceFit's fields, then the limits'.  force_qp.qp_rows reads the same fields."""
    _fields_ = QtosForceFit._fields_ + [
        ("mu", C.c_double), ("f_max", C.c_double), ("mu_end", C.c_double), ("act_tol", C.c_double), ("max_iter", C.c_int),
    ]


def _prototypes():
    """name -> (restype, argtypes) of every entry point, in the header's order.  Host forms take typed pointers, so that a
    numpy array of the wrong dtype is refused here; device forms (and qtos_plan_submit) take c_void_p for every device
    pointer and for the stream, which is what a tensor's data_ptr() converts to."""
    P = C.POINTER
    i, d, q, Q, cp, vp = C.c_int, C.c_double, C.c_longlong, C.c_ulonglong, C.c_char_p, C.c_void_p
    dp, ip, qp, Qp = P(d), P(i), P(q), P(C.c_uint64)
    h = vp                                              # QtosPlanner *: the opaque handle

    def f(*argtypes, ret=i):
        return ret, list(argtypes)
    return {
        "qtos_planner_create": f(P(QtosParams), i, i, P(h)),
        "qtos_planner_destroy": f(h, ret=None),
        "qtos_planner_dims": f(h, P(QtosDims)),
        "qtos_last_error": f(h, ret=cp),
        "qtos_analyze": f(P(QtosParams), P(QtosDims), ip, i),
        "qtos_analyze_sweep": f(P(QtosParams), ip, ip, ip, ip, ip, i),
        "qtos_analyze_order": f(P(QtosParams), ip, i),
        "qtos_analyze_two_ended": f(P(QtosParams), ip, i),
        "qtos_set_heightfields":        f(h, i, dp, i, i, d, d, d),
        "qtos_set_heightfields_device": f(h, i, vp, i, i, d, d, d, vp),
        "qtos_set_init_table": f(h, i, dp, i, dp, dp),
        "qtos_plan_batch":        f(h, i, dp, dp, ip, dp, dp, ip, ip, dp),
        "qtos_plan_batch_device": f(h, i, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_plan_submit":       f(h, i, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_plan_poll": f(h, ip),
        "qtos_plan_wait": f(h),
        "qtos_shift_warm":        f(h, i, dp, dp, dp, dp, ip, dp),
        "qtos_shift_warm_device": f(h, i, vp, vp, vp, vp, vp, vp, vp),
        "qtos_sample_csv":        f(h, i, dp, dp, d, i, dp),
        "qtos_sample_csv_device": f(h, i, vp, vp, d, i, vp, vp),
        "qtos_handover":        f(h, i, P(QtosHandover), dp, dp, dp, dp, dp, ip),
        "qtos_handover_device": f(h, i, P(QtosHandover), vp, vp, vp, vp, vp, vp, vp),
        "qtos_stitch":        f(h, i, P(QtosStitch), dp, ip, dp, dp, qp),
        "qtos_stitch_device": f(h, i, P(QtosStitch), vp, vp, vp, vp, vp, vp),
        "qtos_joint_rows":        f(h, i, P(QtosJointRows), dp, dp, ip, ip, qp, dp, dp, dp, ip),
        "qtos_joint_rows_device": f(h, i, P(QtosJointRows), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_track":        f(h, i, P(QtosTrack), dp, dp, ip, ip, qp, dp, dp, qp, dp, dp, ip),
        "qtos_track_device": f(h, i, P(QtosTrack), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_start_feedback":        f(h, i, P(QtosFeedback), dp, dp, ip, qp, dp, ip, dp, dp, dp, dp, ip),
        "qtos_start_feedback_device": f(h, i, P(QtosFeedback), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_plan_check":        f(h, i, P(QtosPlanCheck), dp, dp, ip, ip, ip, qp, dp, vp),        # (summary: QtosCheckRecord *)
        "qtos_plan_check_device": f(h, i, P(QtosPlanCheck), vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_rollout":        f(h, i, P(QtosRollout), dp, dp, ip, ip, qp, dp, dp, dp, dp, qp, ip, dp, dp, ip),
        "qtos_rollout_device": f(h, i, P(QtosRollout), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_rollout_feet":        f(h, i, P(QtosRolloutFeet), dp, dp, ip, ip, qp, dp, dp, dp, dp, qp, ip, dp, dp, dp, ip),
        "qtos_rollout_feet_device": f(h, i, P(QtosRolloutFeet), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_force_fit":        f(h, i, P(QtosForceFit), dp, dp, ip, ip, ip, qp, dp, dp, dp, ip, vp),   # (summary, as above)
        "qtos_force_fit_device": f(h, i, P(QtosForceFit), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_force_qp":        f(h, i, P(QtosForceQp), dp, dp, ip, ip, ip, qp, dp, dp, dp, dp, ip, vp),
        "qtos_force_qp_device": f(h, i, P(QtosForceQp), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_rollout_qp":        f(h, i, P(QtosRolloutQp), dp, dp, ip, ip, qp, dp, dp, dp, dp, qp, ip, dp, dp, dp, dp, ip),
        "qtos_rollout_qp_device": f(h, i, P(QtosRolloutQp), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_path_goal":        f(h, i, P(QtosPathGoal), dp, dp, ip, dp, ip, dp, ip, dp, dp, dp, dp, ip),
        "qtos_path_goal_device": f(h, i, P(QtosPathGoal), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_path_plan":        f(h, i, P(QtosPathPlan), dp, ip, dp, dp, dp, dp, ip, ip, ip, ip, ip),
        "qtos_path_plan_device": f(h, i, P(QtosPathPlan), vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_probe":        f(h, P(QtosProbe), dp, i, ip, ip, ip, dp, dp, ip),
        "qtos_probe_device": f(h, P(QtosProbe), vp, i, vp, vp, vp, vp, vp, vp, vp),
        "qtos_probe_stamp":        f(h, P(QtosProbe), ip, ip, ip, ip, dp),
        "qtos_probe_stamp_device": f(h, P(QtosProbe), vp, vp, vp, vp, vp, vp),
        "qtos_terrain_env":        f(h, P(QtosTerrainEnv), dp, ip, Qp, ip, dp, dp, ip),
        "qtos_terrain_env_device": f(h, P(QtosTerrainEnv), vp, vp, vp, vp, vp, vp, vp, vp),
        "qtos_write_csv": f(cp, dp, i, i),
        "qtos_set_speculation": f(h, i),
        "qtos_set_pattern_speculation": f(h, i),
        "qtos_env": f(h, cp, i),
        "qtos_last_timing": f(h, dp, ip, dp, ip),
        "qtos_last_timing_detail": f(h, dp, i),
        "qtos_last_timing_chord": f(h, dp, ip),
        "qtos_set_kernel_events": f(h, i),
        "qtos_set_report": f(h, i),
        "qtos_plan_report": f(h, i, P(QtosReport), dp, i),
        "qtos_plan_totals": f(h, qp, qp, i),
        "qtos_analyze_counts": f(P(QtosParams), qp, i),
        "qtos_debug_eval": f(h, i, dp, dp, ip, dp, dp, dp),
        "qtos_debug_newton": f(h, i, dp, dp, ip, dp, dp, dp, dp),
        "qtos_debug_chord": f(h, i, dp),
        "qtos_project_nodes": f(h, i, dp, dp),
        "qtos_debug_stream_len": f(h),
        "qtos_debug_read_stream": f(h, i, dp),
        "qtos_debug_read_rhs": f(h, i, dp),
        "qtos_debug_residual": f(h, i, i, dp, dp),
        "qtos_debug_structure": f(h, ip, ip, ip),
        "qtos_debug_factor": f(h, i, dp, ip),
        "qtos_debug_initial_guess": f(h, i, dp, dp, ip, dp),
        "qtos_debug_trace": f(h, i, dp),
        "qtos_debug_duals": f(h, i, dp, dp, dp, dp),
        "qtos_build_flags": f(),
        "qtos_kkt_kernel": f(h, cp, i),
        "qtos_analyze_kernel": f(P(QtosParams), cp, i),
        "qtos_planner_selftest": f(h, Q, d, P(QtosSelftest)),
        "qtos_planner_create_checked": f(P(QtosParams), i, i, i, d, P(h), P(QtosSelftest), i, ip),
        "qtos_analyze_candidates": f(P(QtosParams), i, ip, ip, ip, i),
        "qtos_selftest_inputs": f(P(QtosParams), Q, i, dp, dp, dp),
        "qtos_selftest_bits": f(Q, i, i, Q, ret=Q),
        "qtos_selftest_problem": f(P(QtosParams), dp, dp),
    }


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)
