// planner_create.hpp -- how a handle comes to be: create_planner, behind qtos_planner_create and the candidates of
// qtos_planner_create_checked.  A part of qtos_planner.hip, included inside its extern "C" block, behind the handle
// (QtosPlanner), HIPCHK, the kernel selectors (kkt2_kernel .. chord_kernel) and choose_kernel.
//
// The handle is built in five steps, in this order (a later step reads what an earlier one wrote): the plan's device tables,
// the solve and evaluation kernels, the sampler's plan, the workspace, the lanes.  A step takes the handle, returns the C ABI's
// code and leaves its reason in the handle's err; create_planner prints it, in one place.  No step frees anything: the handle
// owns what it has allocated (~QtosPlanner), create_planner holds it by a unique_ptr until it hands it out.  Inside a step the
// first upload or allocation that fails sets rc and the later ones are left out, as in Staging.

// err from a format; returns the code to leave with
static int create_error(QtosPlanner *p, int code, const char *fmt, ...) {
  char text[256];
  va_list ap;
  va_start(ap, fmt); vsnprintf(text, sizeof(text), fmt, ap); va_end(ap);
  p->err = text;
  return code;
}
// a HIP call whose failure has one code whatever the error (HIPCHK tells out of memory from the rest)
#define HIPCHK_AS(p, code, call) \
  do { hipError_t e_ = (call); if (e_ != hipSuccess) return create_error(p, code, "%s: %s", #call, hipGetErrorString(e_)); } while (0)

// The rows of the inequality blocks for the helper waves of the backward sweep (sweep_backward): a block belongs to the stage
// of its earliest column; rounds of SW_ROUND rows (one helper wave), round i in step i of the chain (stage NS - 1 - i): a
// stage's rounds come behind the step that solves it, in the order the chain meets the stages.  Returns the number of
// rounds (0: the tables cannot be built for this plan).
static int build_sweep_tasks(const HostModel &M, const Symbolic &S, std::vector<SwTask> &tasks, std::vector<int> &cpos, std::vector<int> &c16) {
  const int NS = S.n_stages;
  std::vector<std::vector<SwTask>> by_stage(NS);
  bool ok = true;
  for (const Block &b : M.blocks) {
    if (b.kind != 1) continue;
    int mn = INT_MAX;
    const int c0 = (int)cpos.size();
    for (int a = 0; a < b.n; ++a) {
      const int pos = S.var_pos[M.block_cols[b.col_off + a]];
      if (pos < 0) ok = false;
      cpos.push_back(std::max(pos, 0));
      mn = std::min(mn, pos);
    }
    if (mn < 0 || mn / PIV >= NS) { ok = false; continue; }
    const int k0 = (int)c16.size(), n4 = b.n & ~3;
    auto at = [&](int e) { return (unsigned)cpos[c0 + e] & 0xffffu; };
    for (int q = 0; q < 4; ++q)
      for (int u = 0; u < SW_RU; u += 2) {
        const int e0 = std::max(std::min(q + 4 * u, n4 - 4 + q), 0), e1 = std::max(std::min(q + 4 * (u + 1), n4 - 4 + q), 0);
        c16.push_back((int)(at(std::min(e0, b.n - 1)) | (at(std::min(e1, b.n - 1)) << 16)));
      }
    {
      const int r0 = std::min(n4, b.n - 1), r1 = std::min(n4 + 1, b.n - 1), r2 = std::min(n4 + 2, b.n - 1);
      c16.push_back((int)(at(r0) | (at(r1) << 16)));
      c16.push_back((int)at(r2));
      c16.push_back(0); c16.push_back(0);
    }
    for (int r = 0; r < b.m; ++r) by_stage[mn / PIV].push_back({b.goff + r * b.n, b.n, b.row0 + r, k0, c0, {0, 0, 0}});
  }
  if ((size_t)NS * PIV > 65535) ok = false;
  const SwTask none = {0, 4, -1, 0, 0, {0, 0, 0}};
  int step = 0;
  auto round_of = [&](const SwTask *t, int cnt) {
    for (int i = 0; i < SW_ROUND; ++i) tasks.push_back(i < cnt ? t[i] : none);
    ++step;
  };
  for (int u = NS - 1; u >= 0 && ok; --u) {
    while (step < NS - u) round_of(nullptr, 0);   // (x of stage u is complete behind the barrier of step NS - 1 - u)
    for (size_t i = 0; i < by_stage[u].size(); i += SW_ROUND) round_of(by_stage[u].data() + i, (int)std::min<size_t>(SW_ROUND, by_stage[u].size() - i));
  }
  const int nstep = ((NS + SWD - 1) / SWD) * SWD;
  while (step < nstep) round_of(nullptr, 0);
  if (cpos.empty()) cpos.push_back(0);
  while (c16.size() < 20) c16.push_back(0);
  if (S.env.debug) {
    size_t mx = 0, tot = 0;
    for (auto &v : by_stage) { mx = std::max(mx, v.size()); tot += v.size(); }
    fprintf(stderr, "qtos: sweep ds: %d rounds for %d stages (chain %d steps), %zu rows, most in a stage %zu; rows by stage:", step, NS, nstep, tot, mx);
    for (auto &v : by_stage) fprintf(stderr, " %zu", v.size());
    fprintf(stderr, "\n");
  }
  return ok ? step : 0;
}

// The spline inputs of n_inst instance structs as flat tables in pre-pass order (the n_vec VecIn records lead each struct):
// per record and component the four variables, and the four weights as two pairs.
static int upload_vec_inputs(QtosPlanner *p, const void *inst0, size_t inst_bytes, size_t n_inst, int n_vec, const i4_t **var, const d2_t **wa, const d2_t **wb) {
  std::vector<i4_t> v; std::vector<d2_t> a, b;
  for (size_t i = 0; i < n_inst; ++i)
    for (int k = 0; k < n_vec; ++k) {
      const VecIn &in = ((const VecIn *)((const char *)inst0 + i * inst_bytes))[k];
      for (int d = 0; d < 3; ++d) {
        v.push_back(i4_t{in.var[d], in.var[3 + d], in.var[6 + d], in.var[9 + d]});
        a.push_back(d2_t{in.w[0], in.w[1]});
        b.push_back(d2_t{in.w[2], in.w[3]});
      }
    }
  int rc = p->upload(v, var);
  if (!rc) rc = p->upload(a, wa);
  if (!rc) rc = p->upload(b, wb);
  return rc;
}
// The entry lists of the iterate-dependent Jacobian values, packed (model.hpp: PackedTerm1 / PackedTerm3): stream offsets of
// 16 bits, and each coefficient as a 16-bit index into the table of the distinct ones.  -4 where either does not fit.
static int upload_jacobian_lists(QtosPlanner *p) {
  const Symbolic &S = p->S; DevPlan &D = p->dp;
  std::map<unsigned long long, int> idx_of;
  std::vector<double> coefs;
  bool fits = true;
  auto ci = [&](double a) {
    unsigned long long bits;
    std::memcpy(&bits, &a, 8);
    auto it = idx_of.find(bits);
    if (it == idx_of.end()) { it = idx_of.emplace(bits, (int)coefs.size()).first; coefs.push_back(a); }
    return (unsigned short)it->second;
  };
  auto off16 = [&](int off) { if (off < 0 || off > 65535) fits = false; return (unsigned short)off; };
  std::vector<PackedTerm1> d1, r1; std::vector<PackedTerm3> d3;
  for (const LinTerm1 &t : S.dyn_t1) d1.push_back({(unsigned)t.pos, off16(t.off), ci(t.a)});
  for (const LinTerm1 &t : S.rom_t1) r1.push_back({(unsigned)t.pos, off16(t.off), ci(t.a)});
  for (const LinTerm3 &t : S.dyn_t3)
    d3.push_back({(unsigned)t.pos, {off16(t.off[0]), off16(t.off[1]), off16(t.off[2])}, {ci(t.a[0]), ci(t.a[1]), ci(t.a[2])}});
  if (!fits || coefs.size() > 65535) return create_error(p, -4, "Jacobian entry lists exceed the packed format (16-bit offsets / coefficient indices)");
  D.n_lin_coef = (int)coefs.size();
  int rc = p->upload(d1, &D.dyn_t1);
  if (!rc) rc = p->upload(d3, &D.dyn_t3);
  if (!rc) rc = p->upload(r1, &D.rom_t1);
  if (!rc) rc = p->upload(coefs, &D.lin_coef);
  return rc;
}
// The terrain rows with their stream positions: the row's Jacobian entries, and the pivot diagonals of the foot node's x and
// y (two-phase solve: stance rows only).
static int upload_terrain_rows(QtosPlanner *p) {
  const HostModel &M = p->M; const Symbolic &S = p->S;
  std::vector<int> dpos_of_var(M.n_sol, -1);
  for (int i = 0; i < (int)S.pack_src.size(); ++i)
    if ((S.pack_src[i] >> 28) == 5) {
      const int u = S.piv_unknown[S.pack_src[i] & 0x0fffffff];
      if (u >= 0 && u < M.n_sol) dpos_of_var[u] = i;
    }
  std::vector<TerrDev> td;
  for (const TerrInst &t : M.terr) {
    TerrDev d = {t.vx, t.vy, t.vz, t.row, -1, -1, -1, -1, -1, 0, 0.0, 0.0};
    if (t.in_kkt) {
      const bool stance = M.row_kind[t.row] == 1;   // equality block: entries at their own stream positions
      auto pos = [&](int c) { return c < 0 ? -1 : (stance ? S.eq_pos[t.goff + c] : t.goff + c); };
      d.px = pos(t.cx); d.py = pos(t.cy); d.pz = pos(t.cz);
      if (M.P.hold_from > 0 && stance) {
        d.d0 = dpos_of_var[t.vx]; d.d1 = dpos_of_var[t.vy];
        d.ex = M.sol_diag[t.vx] - M.P.delta_x; d.ey = M.sol_diag[t.vy] - M.P.delta_x;
      }
    }
    td.push_back(d);
  }
  return p->upload(td, &p->dp.terr);
}

// Step 1: DevPlan, the model and its symbolic analysis as the kernels read them.
static int upload_plan_tables(QtosPlanner *p) {
  const HostModel &M = p->M; const Symbolic &S = p->S; DevPlan &D = p->dp;
  {  // k_step writes a recovered node step next to the coefficient steps it is formed from: the two sets must not meet
    std::vector<char> is_rec(M.n_sol, 0);
    for (int v : M.rec_var) is_rec[v] = 1;
    for (int c : M.rec_col)
      if (c >= 0 && is_rec[c]) return create_error(p, -1, "reduced base: a recovered node value is the source of another");
  }
  int rc = 0;
  auto up = [&](const auto &v, auto out) { if (!rc) rc = p->upload(v, out); };
  std::memset(&D, 0, sizeof(D));
  D.n_vars = M.n_vars; D.n_cons = M.n_cons; D.n_stages = S.n_stages; D.front = S.front;
  D.n_sol = M.n_sol; D.n_rec = (int)M.rec_var.size();
  D.n_coef = M.reduce_base ? M.n_coef : 0; D.n_pz = (int)M.pz_var.size(); D.n_psw = (int)M.psw_var.size();
  up(M.rec_var, &D.rec_var); up(M.rec_col, &D.rec_col); up(M.rec_w, &D.rec_w); up(M.pc_var, &D.pc_var); up(M.pc_w, &D.pc_w);
  up(M.psw_var, &D.psw_var); up(M.psw_src, &D.psw_src); up(M.psw_w, &D.psw_w);
  up(M.pz_var, &D.pz_var); up(M.pz_col, &D.pz_col); up(M.pz_w, &D.pz_w);
  D.n_dyn = (int)M.dyn.size(); D.n_rom = (int)M.rom.size(); D.n_terr = (int)M.terr.size();
  D.n_force = (int)M.force.size(); D.n_lin = (int)M.linrow.size(); D.n_blocks = (int)M.blocks.size();
  up(M.dyn, &D.dyn); up(M.rom, &D.rom);
  static_assert(DYN_VIN == 39 && ROM_VIN == 9, "13 / 3 input vectors of three components");
  if (!rc) rc = upload_vec_inputs(p, M.dyn.data(), sizeof(DynInst), M.dyn.size(), 13, &D.pre_dyn_var, &D.pre_dyn_wa, &D.pre_dyn_wb);
  if (!rc) rc = upload_vec_inputs(p, M.rom.data(), sizeof(RomInst), M.rom.size(), 3, &D.pre_rom_var, &D.pre_rom_wa, &D.pre_rom_wb);
  up(M.force, &D.force); up(M.linrow, &D.lin);
  if (!rc) rc = upload_jacobian_lists(p);
  up(S.dyn_t1_off, &D.dyn_t1_off); up(S.dyn_t3_off, &D.dyn_t3_off);
  D.n_rom_t1 = (int)S.rom_t1.size(); D.dyn_chunk = M.dyn_chunk; D.rom_chunk = S.rom_chunk;
  up(S.rom_t1_off, &D.rom_t1_off); up(S.amask, &D.amask); up(S.amask2, &D.amask2);
  up(S.nxt_pack, &D.nxt_pack); up(S.ctab, &D.ctab); up(S.rtab, &D.rtab);
  up(S.rhs_ptr, &D.rhs_ptr); up(S.rhs_gpos, &D.rhs_gpos); up(S.rhs_row, &D.rhs_row);
  up(S.kx_ptr, &D.kx_ptr); up(S.kx_col, &D.kx_col); up(S.kx_pos, &D.kx_pos);
  D.n_unknowns = S.n_unknowns; D.n_cells = S.n_cells; D.n_cont = S.n_continuation();
  D.chord_tol = M.P.chord_tol;
  D.chord_max = M.P.chord_max > 0 ? M.P.chord_max : 1;
  D.chord_shrink = M.P.chord_shrink > 0 ? M.P.chord_shrink : 1.0 / 3.0;
  D.off_lin = M.off_lin; D.off_ang = M.off_ang;
  for (int e = 0; e < NEE; ++e) D.off_eem[e] = M.off_eem[e];
  up(S.cont, &D.cont);
  if (!rc) rc = upload_terrain_rows(p);
  D.hold_from = M.P.hold_from; D.hold_tol = M.P.hold_tol; D.hold_weight = M.P.hold_weight > 0 ? M.P.hold_weight : 1e6;
  D.spec_jac = p->env.spec_jac;
  up(M.blocks, &D.blocks); up(M.block_cols, &D.block_cols);
  {
    std::vector<IqRow> rows;   // blocks carry their stream offsets once the symbolic analysis has run
    for (const Block &b : M.blocks)
      if (b.kind == 1)
        for (int r = 0; r < b.m; ++r) rows.push_back({b.goff + r * b.n, b.n, b.col_off, b.row0 + r});
    D.n_iq_rows = (int)rows.size();
    up(rows, &D.iq_rows);
  }
  {
    std::vector<SwTask> tasks;
    std::vector<int> cpos, c16;
    D.sw_steps = build_sweep_tasks(M, S, tasks, cpos, c16);
    D.sw_on = D.sw_steps > 0 && D.n_iq_rows > 0 && S.front / PIV < SW_W0 && p->env.sweep_ds != 0;   // (waves 13 .. 15 must be without rows)
    up(tasks, &D.sw_tasks); up(cpos, &D.sw_cpos); up(c16, &D.sw_c16);
  }
  {
    std::vector<int> iq, eq;
    std::vector<double> lo, hi;
    for (int r = 0; r < M.n_cons; ++r) {
      if (M.row_kind[r] == 2) { iq.push_back(r); lo.push_back(M.con_lo[r]); hi.push_back(M.con_hi[r]); }
      else if (M.row_kind[r] == 1) eq.push_back(r);
    }
    D.n_iq = (int)iq.size(); D.n_eqw = (int)eq.size();
    up(iq, &D.iq_idx); up(eq, &D.eq_idx); up(lo, &D.iq_lo); up(hi, &D.iq_hi);
  }
  up(M.g_static, &D.g_static);
  up(S.piv_slot, &D.piv_slot); up(S.piv_unknown, &D.piv_unknown); up(S.piv_diag, &D.piv_diag); up(S.stages, &D.stages);
  up(S.eq_entries, &D.eq_entries); up(S.eq_rhs, &D.eq_rhs); up(S.iq_blocks, &D.iq_blocks); up(S.iq_slots, &D.iq_slots);
  up(M.con_lo, &D.con_lo); up(M.con_hi, &D.con_hi); up(M.row_kind, &D.row_kind); up(M.init, &D.init);
  up(M.node_time, &D.var_time);   // (node times, not the order's keys: model.hpp node_time)
  D.max_stage_g = S.max_stage_g;
  up(S.srec, &D.srec); up(S.srec_off, &D.srec_off); up(S.pack_src, &D.pack_src); up(S.drec_off, &D.drec_off);
  up(S.diag_pos, &D.diag_pos); up(S.pair_groups, &D.pair_groups);
  up(S.eq_pos, &D.eq_pos); up(S.rhs_pos, &D.rhs_pos); up(S.sig_pos, &D.sig_pos); up(S.w_pos, &D.w_pos);
  D.max_srec = S.max_srec; D.max_drec = S.max_drec; D.stream_len = (int)S.pack_src.size();
  D.mass = M.P.mass; D.gravity = M.P.gravity; D.mu_fric = M.P.mu; D.f_max = M.P.f_max; D.T = M.T;
  for (int i = 0; i < 9; ++i) D.Ib[i] = M.P.inertia_b[i];
  for (int e = 0; e < NEE; ++e)
    for (int d = 0; d < 3; ++d) D.nominal[e][d] = M.P.nominal_stance[e][d];
  D.tol = M.P.tol; D.mu_init = M.P.mu_init; D.mu_min = M.P.mu_min; D.delta_x = M.P.delta_x;
  D.mu_superlinear = M.P.mu_superlinear != 0;
  D.eps_dual = M.P.eps_dual; D.max_iter = M.P.max_iter; D.stall_iters = M.P.stall_iters; D.stall_alpha = M.P.stall_alpha;
  D.kappa_sigma = M.P.kappa_sigma;
  D.slack_push = M.P.slack_push > 0 ? M.P.slack_push : 0.01;
  D.warm_slack_push = M.P.warm_slack_push > 0 ? M.P.warm_slack_push : 0.01;
  D.terrain_mode = M.P.terrain_mode;
  D.g_doubles = S.g_doubles;
  D.panel_stride = (long long)S.n_stages * (S.front + 1) * PIV;
  return rc;
}

static int set_dynamic_lds(QtosPlanner *p, const void *fn, size_t bytes) {
  HIPCHK_AS(p, -2, hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}
// Step 2: the LDS of the solve and evaluation kernels, the sweep's helper waves on or off, the kernels' instantiations for
// this front and their dynamic LDS limits.
static int configure_kernels(QtosPlanner *p) {
  const HostModel &M = p->M; const Symbolic &S = p->S; DevPlan &D = p->dp;
  const int F = S.front;
  p->kkt_lds = kkt_lds_bytes(p->kkt, S);
  if (p->kkt == Kkt::kkt5 && F > 128) D.sw_on = 0;   // (nine tile waves of twelve: fewer than three helper waves are left)
  if (D.sw_on) {
    // the helper waves' tables of the backward sweep (solution by position, rounds) behind the sweep's own: within the LDS
    // the forward pass needs anyway, or the kernel's allocation grows up to the limit; beyond that k_step forms ds itself
    const size_t need = (p->kkt == Kkt::kkt5 ? Kkt5Lds::of(F).sweep_base_bytes(S.n_stages) : Kkt2Lds::of(F).sweep_base_bytes(S.n_stages)) + sweep_ds_lds_bytes(S.n_stages, D.sw_steps);
    if (need > LDS_LIMIT || chord_lds_bytes(S.n_stages, D.sw_steps) > 96 * 1024) D.sw_on = 0;
    else p->kkt_lds = std::max(p->kkt_lds, need);
  }
  p->kkt_threads = p->kkt == Kkt::kkt5 ? KT5 : KT2;
  const int max_front = 208;
  if (p->kkt != Kkt::kkt5 && (S.max_drec > 2 * 2 * KT || S.max_srec > 3 * 4 * KT || F > max_front || (S.pack_src.size() & 1)))
    return create_error(p, -4, "stage records too long (%d doubles, %d ints) or front %d > %d: beyond the prefetch registers", S.max_drec, S.max_srec, F, max_front);
  if (p->env.debug) fprintf(stderr, "qtos: front %d, k_kkt LDS %zu B\n", F, p->kkt_lds);
  if (p->kkt_lds > LDS_LIMIT) return create_error(p, -4, "front %d needs %zu B of LDS: too large", F, p->kkt_lds);
  switch (p->kkt) {
    case Kkt::kkt5: p->kkt_fn = kkt5_kernel(F); break;
    case Kkt::kkt3: p->kkt_fn = kkt3_kernel(F); break;
    case Kkt::kkt2: p->kkt_fn = kkt2_kernel(F, D.n_cont > 0); break;
  }
  p->chord_fn = chord_kernel(F);
  if (!p->kkt_fn) return create_error(p, -4, "no k_kkt instantiation for a front of %d", F);
  int rc = set_dynamic_lds(p, (const void *)p->kkt_fn, p->kkt_lds);
  if (!rc && p->chord_fn && D.sw_on) rc = set_dynamic_lds(p, (const void *)p->chord_fn, chord_lds_bytes(S.n_stages, D.sw_steps));
  if (rc) return rc;
  p->eval_lds = sizeof(double) * (((size_t)M.n_sol + 1) / 2 * 2 + std::max((size_t)DYN_LOC * D.dyn_chunk, (size_t)ROM_LOC * D.rom_chunk) +
                                  std::max((size_t)DYN_VIN * D.dyn_chunk, (size_t)ROM_VIN * D.rom_chunk));
  // the coefficient table of the entry lists joins the scratch when it fits (schedules with irregular phase durations have
  // ten thousand distinct Hermite weights: those read it from memory)
  D.coef_in_lds = p->eval_lds + sizeof(double) * (size_t)D.n_lin_coef <= 150 * 1024;
  if (D.coef_in_lds) p->eval_lds += sizeof(double) * (size_t)D.n_lin_coef;
  {  // k_step's pass over the chord right-hand side: unknown sums and list bounds, then the factors of rhs_chunk entries
    D.n_rhs_ent = (int)S.rhs_gpos.size();
    const size_t nuk = (size_t)S.n_unknowns, fixed = ((nuk + 1) & ~(size_t)1) + ((nuk + 4) & ~(size_t)3) / 2;
    const size_t room = 150 * 1024 / sizeof(double) > fixed ? (150 * 1024 / sizeof(double) - fixed) / (2 * (size_t)ET) : 0;   // passes of ET entries that fit
    D.rhs_chunk = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>((D.n_rhs_ent + ET - 1) / ET, 12), room)) * ET;
    p->eval_lds = std::max(p->eval_lds, (fixed + 2 * (size_t)D.rhs_chunk) * sizeof(double));
  }
  if (p->eval_lds > 150 * 1024) return create_error(p, -4, "evaluation kernels need %zu B of LDS: too many dynamics knots for the LDS scratch", p->eval_lds);
  for (const void *fn : {(const void *)k_start, (const void *)k_step, (const void *)k_debug_eval})
    if (!rc) rc = set_dynamic_lds(p, fn, p->eval_lds);
  // (k_probe: the widest map the checks of probe_args admit, one row of 16384 columns, needs a little more than 64 KiB)
  if (!rc) rc = set_dynamic_lds(p, (const void *)k_probe, probe_lds_bytes(1, PP_GRID));
  return rc;
}

static int upload_spline(QtosPlanner *p, const Spline &S, SampleSpline *out) {
  std::vector<double> tend(2 * S.n_polys), dur(S.dur);
  double t = 0;
  double start = 0, start_err = 0;   // the exact start of polynomial i as a sum of two doubles (the additions' rounding errors kept)
  for (int i = 0; i < S.n_polys; ++i) {
    t += S.dur[i];
    tend[i] = t;
    const double start_f64 = tend[i] - S.dur[i];   // the start as sample_spline forms it
    tend[S.n_polys + i] = (start - start_f64) + start_err;
    const double sum = start + S.dur[i], b = sum - start;
    start_err += (start - (sum - b)) + (S.dur[i] - b);
    start = sum;
  }
  std::vector<int> idx;
  for (auto &nd : S.idx)
    for (int i = 0; i < 6; ++i) idx.push_back(nd[i]);
  out->n_polys = S.n_polys;
  int rc = p->upload(tend, &out->tend);
  if (!rc) rc = p->upload(dur, &out->dur);
  if (!rc) rc = p->upload(idx, &out->idx);
  return rc;
}
// Step 3: SamplePlan, the splines as the sampler and the window kernels read them: in the handle, in device memory (d_sp),
// and which polynomials of a foot's motion are stance (d_stance).
static int upload_sample_plan(QtosPlanner *p) {
  const HostModel &M = p->M; SamplePlan &SP = p->sp;
  std::memset(&SP, 0, sizeof(SP));
  SP.n_vars = M.n_vars; SP.T = M.T;
  int rc = upload_spline(p, M.lin, &SP.lin);
  if (!rc) rc = upload_spline(p, M.ang, &SP.ang);
  for (int e = 0; e < NEE; ++e) {
    if (!rc) rc = upload_spline(p, M.eem[e], &SP.eem[e]);
    if (!rc) rc = upload_spline(p, M.eef[e], &SP.eef[e]);
  }
  if (!rc) rc = p->alloc(&p->d_sp, 1);
  if (rc) return rc;
  HIPCHK(p, hipMemcpy(p->d_sp, &SP, sizeof(SP), hipMemcpyHostToDevice));
  for (int e = 0; e < NEE; ++e) {   // a stance polynomial of a foot's motion: neither of its nodes has a velocity variable
    std::vector<int> stance(M.eem[e].n_polys);
    for (int k = 0; k < M.eem[e].n_polys; ++k) stance[k] = M.eem[e].idx[k][3] < 0 && M.eem[e].idx[k + 1][3] < 0;
    if (!rc) rc = p->upload(stance, &p->d_stance[e]);
  }
  return rc;
}

// Step 4: DevWork for max_batch problems, the staging buffers of the host-pointer entry points, their stream and the totals.
static int alloc_workspace(QtosPlanner *p) {
  const HostModel &M = p->M; const Symbolic &S = p->S;
  DevWork &W = p->wk;
  std::memset(&W, 0, sizeof(W));
  const size_t Bm = (size_t)p->max_batch, n = M.n_vars, m = M.n_cons;
  int rc = 0;
  auto al = [&](auto out, size_t count) { if (!rc) rc = p->alloc(out, count); };
  al(&W.x, Bm * n); al(&W.dx, Bm * (size_t)M.n_sol);
  al(&W.g, Bm * m); al(&W.gt, Bm * m); al(&W.s, Bm * m); al(&W.zl, Bm * m); al(&W.zu, Bm * m); al(&W.ds, Bm * m);
  al(&W.dzl, Bm * m); al(&W.dzu, Bm * m); al(&W.sig, Bm * m); al(&W.w, Bm * m);
  al(&W.panel, Bm * (size_t)p->dp.panel_stride);
  al(&W.stream, Bm * (size_t)S.pack_src.size() + 64);   // (+ 64: the helper waves of the sweep read whole groups of a row's entries, sw_load)
  if (rc) return rc;
  {  // constants of the stream (static Jacobian values, pivot diagonals): written once per problem
    std::vector<double> one(S.pack_src.size(), 0.0);
    for (size_t i = 0; i < S.const_pos.size(); ++i) one[S.const_pos[i]] = S.const_val[i];
    for (size_t b = 0; b < Bm; ++b)
      HIPCHK(p, hipMemcpy(W.stream + b * one.size(), one.data(), one.size() * sizeof(double), hipMemcpyHostToDevice));
  }
  al(&W.mu, Bm); al(&W.viol, Bm); al(&W.best_viol, Bm); al(&W.best_it, Bm); al(&W.xbest, Bm * n); al(&W.held, Bm);
#ifdef QTOS_STAMPS
  if (!rc && M.P.max_iter < 79) return create_error(p, -1, "diagnostic build (QTOS_STAMPS) parks its stamps in trace rows 16..79: create the planner with max_iter >= 79");
#endif
  al(&W.trace, Bm * (size_t)(M.P.max_iter + 1) * 4);
  al(&W.hist, Bm * (size_t)(M.P.max_iter + 1) * HIST_COLS); al(&W.rep, Bm * (size_t)REP_COLS);
  al(&W.status, Bm); al(&W.iters, Bm); al(&W.done, Bm);
  al(&W.n_active, 4 * 4);   // four counters per lane
  al(&W.chord, Bm); al(&W.chord_run, Bm); al(&W.jam, Bm);
  al(&W.rhs, Bm * (size_t)S.n_unknowns); al(&W.minv, Bm * (size_t)S.n_stages * PIV * PIV);
  al(&W.sol, Bm * (size_t)S.n_stages * PIV); al(&W.sol0, Bm * (size_t)S.n_stages * PIV);
  al(&W.dx0, Bm * (size_t)M.n_sol); al(&W.ur, Bm * m);
  al(&p->d_start, Bm * QTOS_START_DOUBLES); al(&p->d_goal, Bm * 3);
  al(&p->d_nodes, Bm * n); al(&p->d_warm, Bm * n); al(&p->d_map, Bm);
  if (rc) return rc;
  HIPCHK_AS(p, -2, hipStreamCreateWithFlags(&p->own_stream, hipStreamNonBlocking));
  HIPCHK_AS(p, -3, hipMalloc(&p->d_totals, 2 * sizeof(long long)));
  HIPCHK_AS(p, -3, hipMemset(p->d_totals, 0, 2 * sizeof(long long)));
  p->last_stream = p->own_stream;
  return 0;
}

// Step 5: the lanes, one per part of a call that is larger than the GPU -- QTOS_LANES: at most that many; default ONE: measured
// at 1024 problems per call (round 4, profiles/r04_lanes.txt), parts that start together also reach their stragglers together,
// and four lock-step loops of 256 pay four tails where one loop of 1024 pays one (exp_5 75.8 K plans/s on four lanes, 84.0 K
// on two, 84.2 K on one)
static int create_lanes(QtosPlanner *p) {
  // launch slots of a call: its iterations plus the launches some problem sat out (at most one per blind slot)
  SlotLayout &S = p->slots;
  S.max_slots = 2 * p->M.P.max_iter + 2;
  if (S.max_slots >= SAT_OUT_BASE) return create_error(p, -1, "max_iter %d: more launch slots than the sat-out code of a slot holds", p->M.P.max_iter);
  int cus = 256;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, p->device) != hipSuccess || cus < 1) cus = 256;
  p->lane_chunk = cus;
  const int n_lanes = std::max(1, std::min(p->env.lanes, (p->max_batch + cus - 1) / cus));
  p->lanes.resize(n_lanes);
  HIPCHK_AS(p, -2, hipEventCreateWithFlags(&p->ev_in, hipEventDisableTiming));
  for (int j = 0; j < n_lanes; ++j) {
    QtosPlanner::Lane &L = p->lanes[j];
    HIPCHK_AS(p, -3, hipHostMalloc((void **)&L.h_active, S.count_ints() * sizeof(int), hipHostMallocMapped));
    HIPCHK_AS(p, -2, hipHostGetDevicePointer((void **)&L.h_active_dev, L.h_active, 0));
    L.ran.assign(S.max_slots + 1, 0);
    L.kinds_mask = p->chord_fn ? KIND_KKT | KIND_CHORD : KIND_KKT;
    L.d_n_active = p->wk.n_active + 4 * j;
    if (j > 0) HIPCHK_AS(p, -2, hipStreamCreateWithFlags(&L.own, hipStreamNonBlocking));
    HIPCHK_AS(p, -2, hipStreamCreateWithFlags(&L.side, hipStreamNonBlocking));
    for (hipEvent_t *e : {&L.ev_fork, &L.ev_join, &L.ev_done}) HIPCHK_AS(p, -2, hipEventCreateWithFlags(e, hipEventDisableTiming));
    L.ev.resize(S.n_events());
    for (auto &e : L.ev) HIPCHK_AS(p, -2, hipEventCreate(&e));
  }
  return 0;
}

// The planner of qtos_planner_create (order_rule < 0: the automatic choice / QTOS_ORDER) and of the candidates of
// qtos_planner_create_checked (order_rule >= 0), under the environment `env0` as the caller parsed it.
static int create_planner(const QtosParams *params, int max_batch, int device, const QtosEnv &env0, int order_rule, QtosPlanner **out, Analysis *pre = nullptr) {
  if (!params || !out || max_batch < 1 || max_batch >= MAX_BATCH_LIMIT) return -1;   // (call_schedule.hpp: a count of the count word fits its bits)
  *out = nullptr;
  std::unique_ptr<QtosPlanner> owner(new QtosPlanner());   // (whichever way this function is left, the handle goes with it)
  QtosPlanner *p = owner.get();
  p->device = device; p->max_batch = max_batch; p->env = env0;
  p->pattern.on = p->env.spec_pattern != 0;
  if (choose_kernel(*params, p->env, p->kkt, *p, order_rule, pre)) return -1;   // (it has said why)
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) {
    fprintf(stderr, "qtos: no HIP device %d (found %d) -- the planner has no CPU fallback\n", device, ndev);
    return -2;
  }
  const hipError_t e = hipSetDevice(device);
  p->on_device = e == hipSuccess;
  int rc = p->on_device ? 0 : create_error(p, -2, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  if (!rc) rc = upload_plan_tables(p);
  if (!rc) rc = configure_kernels(p);
  if (!rc) rc = upload_sample_plan(p);
  if (!rc) rc = alloc_workspace(p);
  if (!rc) rc = create_lanes(p);
  if (rc) { fprintf(stderr, "qtos: %s\n", p->err.c_str()); return rc; }
  *out = owner.release();
  return 0;
}
#undef HIPCHK_AS
